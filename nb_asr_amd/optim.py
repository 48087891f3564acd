"""The optimisation step of the reference's trainer on the HIP device (``csrc/optim.hip``, ``nbasr_optim_adam_step``).

What the reference does after ``loss.backward()`` (``training/torch/trainer.py:221-225`` and ``:84``) --

    regu = 0.01 * sum(torch.norm(m.conv.weight) for m in model.modules() if isinstance(m, PadConvRelu))   # added to the loss
    torch.nn.utils.clip_grad_norm_(model.parameters(), 5)
    torch.optim.Adam(model.parameters(), lr=1e-4, eps=1e-7).step()

-- is three launches over all parameter tensors here: the regulariser's gradient, the global norm, the clip and Adam's update.

    opt = nb.optim.reference_optimizer(model, lr=1e-4)          # or optim.Adam(params, ..., max_grad_norm=5, weight_norm_coef=0.01, ...)
    loss.backward(); opt.step(); opt.zero_grad()
    opt.last_grad_norm                                          # what clip_grad_norm_ would have returned (0-dim device tensor)

``Adam`` is a ``torch.optim.Optimizer``: schedulers, ``zero_grad``, ``state_dict`` / ``load_state_dict`` work as usual, and its state dict
has the layout of ``torch.optim.Adam``'s (the reference's checkpoints ``{'model', 'optim'}`` load in either direction).  The regulariser's
VALUE is not computed (the reference only reports the un-regularised loss); its gradient is formed inside the step, ``.grad`` is left as
``backward`` wrote it.  There is no CPU path and no fallback.
"""
import numpy as np
import torch

from . import hip

CHUNK = 16384                     # elements one workgroup handles (a multiple of 4: chunk starts keep the tensor's 16-byte alignment)
WEIGHT_NORM = 1                   # NBASR_OPTIM_WEIGHT_NORM

# struct nbasr_optim_tensor / nbasr_optim_chunk (include/nbasr.h)
ROW_DTYPE = np.dtype([('p', '<u8'), ('grad', '<u8'), ('exp_avg', '<u8'), ('exp_avg_sq', '<u8'), ('count', '<i8'), ('flags', '<i4'),
                      ('first_chunk', '<i4'), ('n_chunks', '<i4'), ('step_size', '<f4'), ('bc2_sqrt', '<f4'), ('reserved', '<i4')])
CHUNK_DTYPE = np.dtype([('tensor', '<i4'), ('length', '<i4'), ('offset', '<i8')])
assert ROW_DTYPE.itemsize == 64 and CHUNK_DTYPE.itemsize == 16


def chunk_table(counts, chunk=CHUNK):
    """Chunk list of a tensor set: ``(chunks, first_chunk, n_chunks)`` with ``chunks`` a list of ``(tensor, offset, length)`` that covers
    every element of every tensor exactly once, tensor by tensor and in ascending order, no chunk longer than ``chunk``; tensor ``t`` owns
    ``chunks[first_chunk[t] : first_chunk[t] + n_chunks[t]]`` (an empty tensor owns none)."""
    if chunk < 4 or chunk % 4:
        raise ValueError(f'chunk_table: chunk={chunk} must be a positive multiple of 4')
    chunks, first, n = [], [], []
    for t, count in enumerate(counts):
        count = int(count)
        if count < 0:
            raise ValueError(f'chunk_table: tensor {t} has a negative element count {count}')
        first.append(len(chunks))
        chunks.extend((t, off, min(chunk, count - off)) for off in range(0, count, chunk))
        n.append(len(chunks) - first[-1])
    return chunks, first, n


def bias_corrections(lr, beta1, beta2, step):
    """``(step_size, bc2_sqrt)`` of torch's Adam at step count ``step``, in double as torch computes them."""
    return lr / (1 - beta1 ** step), (1 - beta2 ** step) ** 0.5


def check_parameter(p, name):
    """Refuse (``ValueError`` naming the parameter) what the kernels do not take: anything but a dense contiguous float32 tensor on a HIP
    device."""
    if p.dtype != torch.float32:
        raise ValueError(f'optim.Adam: {name} must be float32 (got {p.dtype})')
    if p.layout != torch.strided or not p.is_contiguous():
        raise ValueError(f'optim.Adam: {name} must be dense and contiguous')
    if not p.is_cuda:
        raise ValueError(f'optim.Adam: {name} must be on a HIP device (got {p.device}); this package has no CPU path')


def check_companion(t, p, what, name):
    """The same for a gradient or a moment ``t`` of parameter ``p``, which must also have ``p``'s device and shape."""
    if t.layout != torch.strided or t.dtype != torch.float32:
        raise ValueError(f'optim.Adam: the {what} of {name} must be dense float32 (got {t.dtype}, {t.layout})')
    if not t.is_contiguous():
        raise ValueError(f'optim.Adam: the {what} of {name} must be contiguous')
    if t.device != p.device or t.shape != p.shape:
        raise ValueError(f'optim.Adam: the {what} of {name} must have its device and shape '
                         f'(got {t.device} {tuple(t.shape)}, want {p.device} {tuple(p.shape)})')


class Adam(torch.optim.Optimizer):
    """Adam with the reference trainer's gradient clipping and weight-norm regulariser folded into the step (module docstring).

    ``max_grad_norm``: ``clip_grad_norm_``'s ``max_norm`` over ALL parameters of the optimiser (None: no clipping);
    ``weight_norm_coef`` / ``weight_norm_params``: the tensors ``w`` whose 2-norm, times the coefficient, is part of the loss.
    Parameters, gradients and state are dense contiguous float32 tensors on one HIP device; anything else is refused with a ``ValueError``
    that names the parameter (``names``: ``{id(parameter): name}`` for those messages; the position in ``params`` otherwise)."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-7, max_grad_norm=None, weight_norm_coef=0.0, weight_norm_params=(),
                 weight_decay=0, amsgrad=False, maximize=False, *, names=None):
        if isinstance(lr, torch.Tensor):
            raise ValueError('optim.Adam: lr must be a number (a tensor lr would have to be read back every step)')
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f'optim.Adam: betas={betas} must both be in [0, 1)')
        if lr < 0.0 or eps < 0.0:
            raise ValueError(f'optim.Adam: lr={lr} and eps={eps} must not be negative')
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f'optim.Adam: max_grad_norm={max_grad_norm} must be positive (None: no clipping)')
        defaults = self.group_defaults(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize)
        self.names = dict(names or {})                    # id(parameter) -> a name for error messages (reference_optimizer: the model's)
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.weight_norm_coef = float(weight_norm_coef)
        self.last_grad_norm = None
        mine = {id(p) for group in self.param_groups for p in group['params']}
        self._weight_norm = set()
        for k, w in enumerate(weight_norm_params):
            if id(w) not in mine:
                raise ValueError(f'optim.Adam: weight_norm_params[{k}] (shape {tuple(w.shape)}) is not among params')
            self._weight_norm.add(id(w))
        self._check_groups()
        index = 0
        for group in self.param_groups:
            for p in group['params']:
                self.names.setdefault(id(p), f'params[{index}] (shape {tuple(p.shape)})')
                self._check_param(p)
                index += 1
        self._device = None
        self._table = self._workspace = None              # device buffers
        self._capacity = (0, 0)
        self._slots = []                                  # pinned staging buffers: [tensor, event of the last copy out of it]
        self._sent_rows = self._sent_counts = None        # what the device table holds: number of rows, element counts behind the chunk list
        self._done = None                                 # event behind the last step's launches (a stream-side wait, never a host one)
        self._chunks = None

    @staticmethod
    def group_defaults(**options):
        """The group's keys and defaults are those of the installed ``torch.optim.Adam``, so a state dict moves between the two."""
        return dict(torch.optim.Adam([torch.zeros(1)], **options).defaults)

    # ---- refusals ------------------------------------------------------------------------------------------------------------------
    def _name(self, p):
        return self.names.get(id(p), f'a parameter of shape {tuple(p.shape)}')

    def _check_groups(self):
        for group in self.param_groups:
            for key in ('weight_decay', 'amsgrad', 'maximize', 'capturable', 'differentiable'):
                if group.get(key):
                    raise ValueError(f'optim.Adam: {key}={group[key]!r} is not supported (the HIP step is plain Adam: no weight decay, '
                                     f'amsgrad, maximize, capturable or differentiable mode)')
            if isinstance(group['lr'], torch.Tensor):
                raise ValueError('optim.Adam: lr must be a number')
        first = self.param_groups[0]
        for group in self.param_groups[1:]:
            if tuple(group['betas']) != tuple(first['betas']) or group['eps'] != first['eps']:
                raise ValueError('optim.Adam: every parameter group must have the same betas and eps (lr may differ)')

    def _check_param(self, p):
        check_parameter(p, self._name(p))

    def _check_like(self, t, p, what):
        check_companion(t, p, what, self._name(p))

    # ---- the step ------------------------------------------------------------------------------------------------------------------
    def _staging(self, nbytes):
        """A pinned buffer no copy is still reading (never waits: a busy one is left alone and another is made)."""
        for slot in self._slots:
            if slot[0].numel() >= nbytes and (slot[1] is None or slot[1].query()):
                return slot
        slot = [torch.empty(max(nbytes, 4096), dtype=torch.uint8, pin_memory=True), None]
        self._slots.append(slot)
        return slot

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_groups()
        beta1, beta2 = (float(b) for b in self.param_groups[0]['betas'])
        eps = float(self.param_groups[0]['eps'])
        params, grads, lrs = [], [], []
        for group in self.param_groups:
            for p in group['params']:
                g = p.grad
                if g is None:
                    continue
                params.append(p)
                grads.append(g)
                lrs.append(float(group['lr']))
        if not params:
            self.last_grad_norm = None
            return loss
        steps, avgs, sqs = [], [], []
        for p, g in zip(params, grads):
            self._check_param(p)
            self._check_like(g, p, 'gradient')
            state = self.state[p]
            if len(state) == 0:
                state['step'] = torch.tensor(0.0, dtype=torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32)
                state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            step = state['step']
            if not isinstance(step, torch.Tensor):                  # (state dicts of old torch versions hold a number)
                step = state['step'] = torch.tensor(float(step))
            if step.is_cuda:
                raise ValueError(f'optim.Adam: the step count of {self._name(p)} is on {step.device} (a capturable optimiser\'s state); '
                                 f'move it to the CPU')
            self._check_like(state['exp_avg'], p, 'exp_avg')
            self._check_like(state['exp_avg_sq'], p, 'exp_avg_sq')
            steps.append(step)
            avgs.append(state['exp_avg'])
            sqs.append(state['exp_avg_sq'])
        device = params[0].device
        for p in params:
            if p.device != device:
                raise ValueError(f'optim.Adam: {self._name(p)} is on {p.device}, other parameters on {device}: one optimiser per device')
        torch._foreach_add_(steps, 1)
        counts_t = [int(t) for t in torch.stack(steps).tolist()]

        # ---- the table: rows (with this step's bias corrections) every step, the chunk list when the element counts changed
        live = [i for i, p in enumerate(params) if p.numel() > 0]    # (an empty tensor has a step count and nothing to update)
        n = len(live)
        if n == 0:
            self.last_grad_norm = torch.zeros((), device=device)
            return loss
        counts = np.fromiter((params[i].numel() for i in live), dtype=np.int64, count=n)
        if self._sent_counts is None or not np.array_equal(counts, self._sent_counts):
            listed, first, n_chunks = chunk_table(counts)
            chunks = np.zeros(len(listed), dtype=CHUNK_DTYPE)
            if listed:
                chunks['tensor'], chunks['offset'], chunks['length'] = (np.array(col) for col in zip(*listed))
            self._chunks = (chunks, np.array(first, dtype=np.int32), np.array(n_chunks, dtype=np.int32))
            new_chunks = True
        else:
            new_chunks = False
        chunks, first, n_chunks = self._chunks
        rows = np.zeros(n, dtype=ROW_DTYPE)
        rows['p'] = [params[i].data_ptr() for i in live]
        rows['grad'] = [grads[i].data_ptr() for i in live]
        rows['exp_avg'] = [avgs[i].data_ptr() for i in live]
        rows['exp_avg_sq'] = [sqs[i].data_ptr() for i in live]
        rows['count'] = counts
        rows['flags'] = [WEIGHT_NORM if id(params[i]) in self._weight_norm else 0 for i in live]
        rows['first_chunk'] = first
        rows['n_chunks'] = n_chunks
        cache = {}
        scalars = []
        for i in live:
            key = (lrs[i], counts_t[i])
            if key not in cache:
                cache[key] = bias_corrections(lrs[i], beta1, beta2, counts_t[i])
            scalars.append(cache[key])
        rows['step_size'] = [s[0] for s in scalars]
        rows['bc2_sqrt'] = [s[1] for s in scalars]

        lib = hip.load_library()
        total_chunks = len(chunks)
        if self._device != device or n > self._capacity[0] or total_chunks > self._capacity[1]:
            cap = (max(n, self._capacity[0]), max(total_chunks, self._capacity[1]))
            self._table = torch.empty(cap[0] * ROW_DTYPE.itemsize + cap[1] * CHUNK_DTYPE.itemsize, dtype=torch.uint8, device=device)
            self._workspace = torch.empty(int(lib.nbasr_optim_workspace_bytes(cap[0], cap[1])), dtype=torch.uint8, device=device)
            self._capacity, self._device = cap, device
            self._sent_rows, new_chunks = None, True
        # The device table of THIS call is rows[n] then chunks[total_chunks] (nbasr.h), whatever the capacity.  The rows carry this
        # step's bias corrections, so they travel every step (one pinned asynchronous copy, 64 bytes per tensor); the chunk list behind
        # them only when the element counts, or the number of rows in front of it, changed.
        if self._sent_rows != n:
            new_chunks = True
        stream = torch.cuda.current_stream(device)
        if self._done is not None:
            stream.wait_event(self._done)        # a step on another stream: the table and workspace of the last one are still in use there
        blob = rows.tobytes() + (chunks.tobytes() if new_chunks else b'')
        slot = self._staging(len(blob))
        slot[0].numpy()[:len(blob)] = np.frombuffer(blob, dtype=np.uint8)
        self._table[:len(blob)].copy_(slot[0][:len(blob)], non_blocking=True)
        slot[1] = slot[1] or torch.cuda.Event()
        slot[1].record(stream)
        self._sent_rows, self._sent_counts = n, counts
        norm = torch.empty((), dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            rc = lib.nbasr_optim_adam_step(self._table.data_ptr(), n, total_chunks, self._workspace.data_ptr(), norm.data_ptr(), beta1, beta2,
                                           eps, self.max_grad_norm or 0.0, self.weight_norm_coef, stream.cuda_stream)
        hip._check(rc, 'nbasr_optim_adam_step')
        self._done = self._done or torch.cuda.Event()
        self._done.record(stream)
        # the kernels wrote behind autograd's back: packed-weight caches and streaming sessions key on the version counter
        torch.autograd.graph.increment_version([params[i] for i in live])
        self.last_grad_norm = norm
        return loss


def reference_optimizer(model, lr=1e-4):
    """The reference trainer's configuration (``trainer.py:84, 221-225``): Adam with eps 1e-7 over every parameter, gradient norm clipped
    to 5, and 0.01 x the 2-norm of every ``PadConvRelu`` convolution weight as regulariser."""
    from .ops import PadConvRelu
    convs = [m.conv.weight for m in model.modules() if isinstance(m, PadConvRelu)]
    named = list(model.named_parameters())
    return Adam([p for _, p in named], lr=lr, eps=1e-7, max_grad_norm=5, weight_norm_coef=0.01, weight_norm_params=convs,
                names={id(p): name for name, p in named})
