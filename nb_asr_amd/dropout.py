"""Training-mode dropout on the counter-based HIP kernel (include/nbasr.h "dropout").

The reference ends every ``PadConvRelu`` / ``Linear`` op in an ``nn.Dropout`` and puts one more in front of the LSTM (ops.py:22,29,40,48,
model.py:99).  With the ``'hip'`` backend those sites run ``nbasr_dropout``: the mask of an element is a pure function of
``(seed, call, row, frame)``, so nothing is saved for backward (it is the same launch on the gradient), a run can be replayed from
``(seed, calls)``, and the forward under ``torch.no_grad()`` draws the masks of the differentiable forward.

    import nb_asr_amd as nb
    nb.dropout.use('hip')                    # process-wide; `with nb.dropout.use('hip'):` restores the previous backend on exit
    nb.dropout.manual_seed(1234)             # calls = 0
    loss = ...; loss.backward()
    state = nb.dropout.get_state()           # (seed, calls): into the checkpoint; set_state(state) resumes onto the same masks

``'aten'`` (the default) leaves every site on ``torch.nn.functional.dropout`` as before.  The fused executor, streaming sessions and bf16
hold no masks in either backend and keep refusing p > 0 in training mode.
"""
import torch

from . import hip

BACKENDS = ('aten', 'hip')

_backend = 'aten'
_seed = None                     # None: torch.initial_seed() at first use (a read: no generator advances)
_calls = 0


class _Use:
    """What ``use`` returns: the backend is already selected; as a context manager it puts the previous one back on exit."""

    def __init__(self, previous):
        self._previous = previous

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        global _backend
        _backend = self._previous
        return False


def use(name):
    """Select the dropout backend of the training path, process-wide: 'aten' (torch.nn.functional.dropout) or 'hip' (nbasr_dropout)."""
    global _backend
    if name not in BACKENDS:
        raise ValueError(f'unknown dropout backend {name!r}: expected one of {BACKENDS}')
    previous, _backend = _backend, name
    return _Use(previous)


def backend():
    return _backend


def manual_seed(seed):
    """Set the seed (a 64-bit pattern; negative values are legal) and the call counter to 0."""
    global _seed, _calls
    _seed, _calls = int(seed), 0


def get_state():
    """(seed, calls): what a checkpoint keeps.  Unseeded, the seed becomes ``torch.initial_seed()`` here."""
    global _seed
    if _seed is None:
        _seed = int(torch.initial_seed())
    return _seed, _calls


def set_state(state):
    global _seed, _calls
    seed, calls = state
    _seed, _calls = int(seed), int(calls)


def _next_call():
    global _calls
    seed, call = get_state()
    _calls = call + 1
    return seed, call


def _pitched(t):
    """(B, C, T) -> ((B, C, ld) tensor, T).  What the ops of autograd.py return when T is no multiple of 4 -- the T-wide slice of a pitched
    buffer -- is taken as that buffer, without a copy: the kernel neither needs nor writes the pitch columns.  Anything else is pitched
    as autograd._pitched does it."""
    b, c, frames = t.shape
    ld = hip.round_up4(frames)
    t = t.detach()
    if (ld != frames and t.stride() == (c * ld, ld, 1) and t.data_ptr() % 16 == 0
            and (t.storage_offset() + b * c * ld) * t.element_size() <= t.untyped_storage().nbytes()):
        return t.as_strided((b, c, ld), (c * ld, ld, 1)), frames
    from .autograd import _pitched as pitched_copy
    return pitched_copy(t)


def _launch(t, p, seed, call, skips=()):
    """One nbasr_dropout launch on the (B, C, T) tensor t: in place on the pitched copy where one had to be made (a tensor that is
    already pitched may be an op's saved output and is only read)."""
    tp, frames = _pitched(t)
    out = torch.empty_like(tp) if tp.data_ptr() == t.data_ptr() else tp
    hip.dropout(tp, out, frames, p, seed, call, [_pitched(s)[0] for s in skips])
    return out[:, :, :frames]


class _Dropout(torch.autograd.Function):
    """y = drop(x) (+ skips); dx = drop(dy) with the same (p, seed, call), every skip's gradient is dy.  Nothing is saved."""

    @staticmethod
    def forward(ctx, x, p, seed, call, *skips):
        ctx.cfg = (p, seed, call, len(skips))
        return _launch(x, p, seed, call, skips)

    @staticmethod
    def backward(ctx, dy):
        p, seed, call, n = ctx.cfg
        dx = _launch(dy, p, seed, call) if ctx.needs_input_grad[0] else None
        return (dx, None, None, None) + (dy,) * n


def dropout(x, p, training=True, skips=()):
    """Dropout of the (B, C, T) float32 device tensor x with rate p, differentiable, plus the node's sum over up to three ``skips``
    (``((drop(x) + skip0) + skip1) + skip2``, one launch).  Each application takes the next call number.  ``not training`` or ``p == 0``:
    the identity (the plain sum, with skips) -- no dropout launch, no counter step."""
    if not 0.0 <= p <= 1.0:
        raise ValueError(f'dropout probability has to be between 0 and 1, but got {p}')
    if len(skips) > 3:
        raise ValueError(f'at most three skips per launch (got {len(skips)})')
    if not training or p == 0:
        if not skips:
            return x
        from .autograd import skip_sum
        return skip_sum([x, *skips])
    if x.dim() != 3:
        raise ValueError(f'expected a (batch, channels, frames) tensor, got shape {tuple(x.shape)}')
    seed, call = _next_call()
    return _Dropout.apply(x, float(p), seed, call, *skips)
