"""The LSTM recurrence (reference model.py:100, 118-121: nn.LSTM, gates i, f, g, o) restated frame by frame in torch on the CPU, in
fp32 or fp64, with an optional carried state; the edge lists of tests/test_recurrent_edges_gpu.py; the one error rule of that file.
No GPU, no test functions.

``recurrence`` is ``oracle.asr_oracle.lstm_forward_loop`` started from the PROJECTED gates (T, B, 4H) -- what every recurrence kernel of
lstm.hip and lstm_xcd.hip is handed -- so that a kernel is compared with the reference's arithmetic on exactly its own input:

    pre = gates[t] + h @ w_hh^T;  i, f, g, o = pre.chunk(4);  c = sigmoid(f) c + sigmoid(i) tanh(g);  h = sigmoid(o) tanh(c)

The rule (``Family``): truth = the fp64 restatement, want = the fp32 restatement (never another HIP kernel); got is held to
cases.FACTORS against truth -- rms error <= 1.5 x the restatement's, per case; worst element <= 2 x the restatement's worst, over the
pooled cases of one edge family (one kernel, one swept axis: a case of a few dozen outputs is too small a sample for its own worst).
"""
import itertools
import math

import torch

import cases

F32, F64 = torch.float32, torch.float64

# ---- the edge lists -------------------------------------------------------------------------------------------------------------------
BASE = (36, 17, 3)                                        # (hidden, batch, frames) every recurrence sweep starts from
# lstm_step_packed_kernel / lstm_seq_kernel: a slice is 8 hidden units, a k-chunk 16, a wave takes 4 chunks, a round is 8 waves x 4 chunks = 512
HIDDEN_F32 = (4, 8, 12, 16, 20, 64, 68, 500, 508, 512, 516, 1024)
HIDDEN_SEQ = tuple(h for h in HIDDEN_F32 if h <= 512)     # the one-launch form: all of K in one round
# lstm_xcd_kernel / lstm_step16_kernel: a slice is 16 hidden units (4 row tiles), a k-step 32, 16 k-steps
HIDDEN_XCD = (4, 8, 12, 16, 20, 28, 32, 36, 60, 64, 68, 500, 508, 512)
BATCHES = (1, 15, 16, 17, 32, 33)                         # a tile is 16 utterances; the priority and WPB switches sit between 32 and 33
BATCH_HIDDEN = (36, 500)                                  # the batch axis is swept at both
FRAMES_F32 = (1, 2, 5)                                    # frame 0 reads neither cell nor h
FRAMES_XCD = (1, 2, 3, 5)                                 # the pre_a / pre_b / pre_c rotation changes shape at 1 | 2 | 3
ALONE_HIDDEN = (12, 500, 516)                             # every utterance of B = 17 alone, bit for bit
STATE_HIDDEN = (4, 36, 500)                               # frames16_state: B = 17, T = 5, split after every frame
SEQ_RESIDENCY = (512, 64)                                 # (hidden, batch): 64 slices x 4 tiles = 256 workgroups, the residency limit

# lstm_input_projection: 128 x 128 tile, K-step 32, the blocked sum flushed every 4 K-steps, time-major store
PROJ_BASE = (36, 36, 5, 3)                                # (c_in, hidden, frames, batch)
PROJ_C_IN = (4, 32, 36, 124, 128, 132, 260)
PROJ_HIDDEN = (4, 32, 36, 500)
PROJ_FRAMES = (1, 127, 128, 129)
PROJ_BATCH = (1, 3)

# head_kernel: a wave owns 16 rows, a workgroup 64; part is folded into acc every 8 chunks = 128 features; classes in 4 tiles of 16
HEAD_BASE = (65, 132, 49)                                 # (rows, features, classes)
HEAD_ROWS = (1, 15, 16, 17, 63, 64, 65)
HEAD_FEATURES = (4, 12, 16, 20, 124, 128, 132, 256, 260, 500, 1200)
HEAD_CLASSES = (1, 15, 16, 17, 48, 49, 63, 64)
HEAD_BCT = ((7, 5), (3, 17))                              # (batch, frames): a wave's 16 rows straddle utterances

# the gate arithmetic: every value in every role, every (g, o) pair
GATE_GRID = (64, 512)                                     # (batch, hidden) of the gate tensor
_CROSS = [0.34 + 0.02 * k / 40 for k in range(41)]        # 41 points across the series-to-rational crossover of lx_tanh
GATE_VALUES = tuple(_CROSS + [-v for v in _CROSS] + [0.0, -0.0, 1e-30, -1e-30, 1e-8]
                    + [s * v for v in (0.1, 1.0, 5.0, 17.0, 30.0, 88.0, 89.0, 104.0, 1e4) for s in (1.0, -1.0)])
assert len(GATE_VALUES) == 105


def w_scale(hidden):
    return 0.1 if hidden >= 500 else 0.3


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def gates_fn(i, f, g, o, c_prev, dtype):
    """One elementwise cell update in ``dtype``: (c, h)."""
    i, f, g, o, c_prev = (v.to(dtype) for v in (i, f, g, o, c_prev))
    c = torch.sigmoid(f) * c_prev + torch.sigmoid(i) * torch.tanh(g)
    return c, torch.sigmoid(o) * torch.tanh(c)


def recurrence(gates, w_hh, dtype, h0=None, c0=None):
    """gates (T, B, 4H) = the input projection with both biases, w_hh (4H, H), any device -> h (B, T, H), c_T (B, H) in ``dtype`` on
    the CPU; ``h0`` / ``c0`` (B, H): the carried state (None: zeros)."""
    gates, w_t = gates.detach().cpu().to(dtype), w_hh.detach().cpu().to(dtype).t().contiguous()
    t_n, b, h4 = gates.shape
    hid = h4 // 4
    h = torch.zeros(b, hid, dtype=dtype) if h0 is None else h0.detach().cpu().to(dtype)
    c = torch.zeros(b, hid, dtype=dtype) if c0 is None else c0.detach().cpu().to(dtype)
    out = torch.empty(b, t_n, hid, dtype=dtype)
    for t in range(t_n):
        i, f, g, o = (gates[t] + h @ w_t).chunk(4, dim=1)
        c, h = gates_fn(i, f, g, o, c, dtype)
        out[:, t] = h
    return out, c


def draw(hidden, batch, frames, seed=0):
    """(gates (T, B, 4H), w_hh (4H, H)) on the CPU; one draw per shape."""
    gen = torch.Generator().manual_seed(hidden * 100003 + batch * 1009 + frames * 17 + seed)
    return torch.randn(frames, batch, 4 * hidden, generator=gen), torch.randn(4 * hidden, hidden, generator=gen) * w_scale(hidden)


def gate_grid(frames):
    """The (frames, B, 4H) gate tensor of the gate-arithmetic test: cell n = b * H + j takes g = V[n % 105], o = V[n // 105 % 105] (every
    pair: 105^2 = 11 025 <= 32 768 cells) and i, f = V at two other strides coprime to 105 (every value in every role).  Every frame
    holds the same gates: c_1 = (1 + sigmoid(f)) c_0 then sums two terms of ONE sign, nothing cancels."""
    b, hid = GATE_GRID
    v = torch.tensor(GATE_VALUES, dtype=F32)
    n = torch.arange(b * hid)
    idx = {'g': n % 105, 'o': (n // 105) % 105, 'i': (2 * n + n // 105) % 105, 'f': (11 * n + 3 * (n // 105) + 1) % 105}
    assert all(len(set(ix.tolist())) == 105 for ix in idx.values()) and len(set((idx['g'] * 105 + idx['o']).tolist())) == 105 * 105
    frame = torch.cat([v[idx[k]].view(b, hid) for k in 'ifgo'], dim=1)
    return frame[None].repeat(frames, 1, 1).contiguous()


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def rms(e):
    return float(e.double().pow(2).mean().sqrt()) if e.numel() else 0.0


class Family:
    """The cases of one edge family (one kernel, one swept axis) under the rule of the module docstring.  ``add`` checks the rms leg of
    one case and pools its errors; ``close`` asserts every case's rms leg and the worst-element leg over the pool.  ``floor`` = (rms, worst) the kernel may add
    to the restatement's error at this case -- (0, 0) unless the kernel documents coarser functions than libm's (derived where it is
    defined, never fitted); the pooled leg takes the largest of its cases' floors."""

    def __init__(self, name):
        self.name = name
        self.worst_got = self.worst_ref = self.ratio_rms = self.floor_worst = 0.0
        self.case_of_ratio, self.failed = None, []

    def add(self, case, got, want, truth, floor=(0.0, 0.0)):
        got, want, truth = (torch.as_tensor(t).detach().double().cpu() for t in (got, want, truth))
        assert got.shape == truth.shape == want.shape, (self.name, case, got.shape, truth.shape)
        assert bool(torch.isfinite(got).all()), (self.name, case, 'non-finite output')
        e_got, e_ref = (got - truth).abs(), (want - truth).abs()
        r_got, r_ref = rms(e_got), rms(e_ref)
        ratio = r_got / max(r_ref, 1e-300)
        print(f'{self.name} | {case}: rms e_gpu {r_got:.3e} e_ref {r_ref:.3e} ratio {ratio:5.2f} | worst e_gpu {float(e_got.max()):.3e} '
              f'e_ref {float(e_ref.max()):.3e} ({got.numel()} outputs)')
        if ratio > self.ratio_rms:
            self.ratio_rms, self.case_of_ratio = ratio, case
        self.worst_got, self.worst_ref = max(self.worst_got, float(e_got.max())), max(self.worst_ref, float(e_ref.max()))
        self.floor_worst = max(self.floor_worst, floor[1])
        if not r_got <= cases.FACTORS[0] * r_ref + floor[0]:          # (asserted in close(): the whole family is measured first)
            self.failed.append(f'{case}: rms error vs fp64 {r_got:.3e}, the restatement {r_ref:.3e}')

    def close(self):
        print(f'{self.name} | FAMILY: worst e_gpu {self.worst_got:.3e} e_ref {self.worst_ref:.3e} ratio '
              f'{self.worst_got / max(self.worst_ref, 1e-300):5.2f} | largest rms ratio {self.ratio_rms:5.2f} at {self.case_of_ratio}')
        assert not self.failed, (self.name, self.failed)
        assert self.worst_got <= cases.FACTORS[1] * self.worst_ref + self.floor_worst, \
            (self.name, 'worst element vs fp64', self.worst_got, 'restatement', self.worst_ref)


def sweeps(hiddens, batches, frames):
    """{axis: [(hidden, batch, frames)]}: one axis at a time around BASE; the batch axis at both widths of BATCH_HIDDEN."""
    h0, b0, t0 = BASE
    return {'hidden': [(h, b0, t0) for h in hiddens],
            'batch': [(h, b, t0) for h, b in itertools.product(BATCH_HIDDEN, batches)],
            'frames': [(h0, b0, t) for t in frames]}


ULP = 2.0 ** -23                                          # the relative size of one fp32 ulp, at most
U1 = 2.0 ** -24                                           # one ulp of a value in [0.5, 1): the absolute size of an ulp of sigmoid or tanh, at most


def xcd_floor(frames):
    """What lstm_xcd.hip's gate functions may add to the restatement's RMS error: ((rms, 0) of h, (rms, 0) of c_T).  The worst-element leg
    gets nothing (measured without it: at most 1.46 x the restatement's worst where 2 x is allowed).

    The kernel documents hardware exp2 / rcp forms at <= 2 ulp per function where libm's are <= 1: one extra ulp per function value,
    and every function value lies in (-1, 1), where an ulp is at most U1 = 2^-24.  h_t = sigmoid(o) tanh(c_t) and
    c_t = sigmoid(f) c_(t-1) + sigmoid(i) tanh(g): four function values of the frame reach h_t with partial derivatives <= 1
    (sigmoid(o), tanh(c), and through c with 1 - tanh^2 <= 1: sigmoid(i), tanh(g)); c_T collects three function values per frame.
    n independent errors, each uniform within +-U1, have the rms U1 sqrt(n / 3): U1 sqrt(4 / 3) = 6.9e-8 for h, U1 sqrt(T) for c_T.
    (What the leg then still sees is a wrong product or a wrong state -- 1e-3 and more, see "Broken by hand" -- the functions
    themselves are held to ulps by the gate-arithmetic test.)"""
    return (U1 * math.sqrt(4 / 3), 0.0), (U1 * math.sqrt(3 * frames / 3), 0.0)
