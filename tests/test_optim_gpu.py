"""nb_asr_amd.optim on the GPU: the HIP step (regulariser gradient + clip_grad_norm_ + Adam) against torch's own recipe.

The parity rule is the project's (tests/cases.py FACTORS): with `truth` the torch recipe in float64 on the CPU and `want` the same in
float32 on the CPU, the kernel's p, exp_avg and exp_avg_sq are no further from `truth` than 1.5 x (rms) / 2.0 x (worst element) the
error of `want` -- measured over all updated tensors of the synthetic set together (131 486 elements; a single-element tensor has no
error statistics of its own).  Each figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import nb_asr_amd as nb
from nb_asr_amd import ctc, ops, optim
from tests.cases import ARCH_A, FACTORS

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CH = optim.CHUNK
LR, EPS, MAX_NORM, COEF = 1e-4, 1e-7, 5.0, 0.01
STEPS = 3
# name, shape, how it is held
SPEC = [('one', (1,), 'plain'), ('three', (3,), 'plain'), ('seven', (7,), 'plain'), ('reg257', (257,), 'plain'), ('below', (CH - 1,), 'plain'),
        ('above', (CH + 1,), 'plain'), ('three_chunks', (2 * CH + 5,), 'plain'), ('reg_zeros', (5, 3, 8), 'plain'), ('frozen', (11,), 'frozen'),
        ('no_grad', (13,), 'none'), ('view9', (9,), 'view'), ('view_two_chunks', (CH + 3,), 'view')]
FLAGGED = ('reg257', 'reg_zeros')
UPDATED = [name for name, _, how in SPEC if how in ('plain', 'view')]


def _values(grad_scale):
    """{name: (p0, [g of every step])} float32 CPU tensors, the same for every run."""
    gen = torch.Generator().manual_seed(20240917)
    out = {}
    for name, shape, _ in SPEC:
        p0 = torch.zeros(shape) if name == 'reg_zeros' else torch.randn(shape, generator=gen)
        out[name] = (p0, [3.0 * grad_scale * torch.randn(shape, generator=gen) for _ in range(STEPS)])
    return out


def _params(values, device, dtype, aligned_views=False):
    """The parameter set of SPEC on `device`: {name: nn.Parameter}, and the flat buffer the 'view' parameters live in at element offset 1
    (4-byte aligned only: the scalar path)."""
    views = [(name, int(np.prod(shape))) for name, shape, how in SPEC if how == 'view']
    flat = torch.full((2 + sum(n + 3 for _, n in views),), 7.0, dtype=dtype, device=device)
    params, at = {}, 0 if aligned_views else 1
    for name, shape, how in SPEC:
        p0 = values[name][0].to(device=device, dtype=dtype)
        if how == 'view':
            n = p0.numel()
            if aligned_views:
                at = (at + 3) // 4 * 4
            flat[at:at + n] = p0
            params[name] = torch.nn.Parameter(flat[at:at + n])
            at += n + (0 if aligned_views else 4 - n % 4)               # keeps the next view at an offset of 1 (mod 4) too
        else:
            params[name] = torch.nn.Parameter(p0.clone(), requires_grad=how != 'frozen')
    return params, flat


def _set_grads(params, values, step):
    for name, _, how in SPEC:
        g = values[name][1][step].to(device=params[name].device, dtype=params[name].dtype)
        params[name].grad = g.clone() if how in ('plain', 'view') else None


def _torch_step(params, opt, max_norm=MAX_NORM):
    """The reference's recipe with torch's own operations; returns what clip_grad_norm_ returned."""
    reg = COEF * sum(torch.norm(params[name]) for name in FLAGGED)
    reg.backward()
    norm = torch.nn.utils.clip_grad_norm_(list(params.values()), max_norm)
    opt.step()
    return norm


def _torch_run(values, device, dtype, steps=STEPS, gamma=None):
    params, _ = _params(values, device, dtype)
    opt = torch.optim.Adam(list(params.values()), lr=LR, eps=EPS)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma) if gamma else None
    norms = []
    for step in range(steps):
        _set_grads(params, values, step)
        norms.append(float(_torch_step(params, opt)))
        if sched:
            sched.step()
    return params, opt, norms


def _hip_optimizer(params):
    return optim.Adam(list(params.values()), lr=LR, eps=EPS, max_grad_norm=MAX_NORM, weight_norm_coef=COEF,
                      weight_norm_params=[params[name] for name in FLAGGED], names={id(p): name for name, p in params.items()})


def _hip_run(values, steps=STEPS, gamma=None, aligned_views=False):
    params, flat = _params(values, DEV, torch.float32, aligned_views)
    opt = _hip_optimizer(params)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma) if gamma else None
    norms = []
    for step in range(steps):
        _set_grads(params, values, step)
        opt.step()
        norms.append(opt.last_grad_norm)
        if sched:
            sched.step()
    return params, opt, norms, flat


def _state(params, opt, key):
    if key == 'p':
        return torch.cat([params[name].detach().reshape(-1).double().cpu() for name in UPDATED])
    return torch.cat([opt.state[params[name]][key].reshape(-1).double().cpu() for name in UPDATED])


def _rms(v):
    return float(v.pow(2).mean().sqrt())


def _assert_rule(got, want, truth, what):
    """cases.FACTORS against the reference's OWN float32 error (never against the code under test)."""
    e_got, e_ref = got - truth, want - truth
    print(f'{what}: rms error vs fp64 {_rms(e_got):.3e} (reference {_rms(e_ref):.3e}), worst {float(e_got.abs().max()):.3e} '
          f'(reference {float(e_ref.abs().max()):.3e}), scale {_rms(truth):.3e}')
    assert _rms(e_ref) > 0 and torch.isfinite(got).all()
    assert _rms(e_got) <= FACTORS[0] * _rms(e_ref), what
    assert float(e_got.abs().max()) <= FACTORS[1] * float(e_ref.abs().max()), what


def _assert_all(got, want, truth, what):
    for key in ('p', 'exp_avg', 'exp_avg_sq'):
        _assert_rule(_state(*got, key), _state(*want, key), _state(*truth, key), f'{what} {key}')


@pytest.fixture(scope='module', params=['clipped', 'not_clipped'])
def case(request):
    """The reference runs (float64 and float32 on the CPU), computed once per gradient scale and left alone."""
    values = _values(1.0 if request.param == 'clipped' else 1e-3)
    truth = _torch_run(values, 'cpu', torch.float64)
    want = _torch_run(values, 'cpu', torch.float32)
    assert (truth[2][0] > MAX_NORM) == (request.param == 'clipped')
    return values, truth, want


def test_three_steps_match_the_torch_recipe(case):
    values, truth, want = case
    params, opt, norms, flat = _hip_run(values)
    _assert_all((params, opt), want[:2], truth[:2], 'three steps')
    for step, (got, ref) in enumerate(zip(norms, truth[2])):
        assert got.dim() == 0 and got.is_cuda and got.dtype == torch.float32
        ulp = float(np.spacing(np.float32(ref)))
        print(f'step {step}: grad norm {float(got):.9g}, fp64 {ref:.12g}, ulp {ulp:.3g}')
        assert abs(float(got) - ref) <= 2 * ulp
    for name in UPDATED:                                                                          # torch's state layout
        state = opt.state[params[name]]
        assert set(state) == {'step', 'exp_avg', 'exp_avg_sq'} and float(state['step']) == STEPS and not state['step'].is_cuda
        assert params[name]._version >= STEPS
    # what must not move, to the bit: the frozen parameter, the one without a gradient, the flat buffer around the views, every .grad
    p0 = {name: values[name][0].to(DEV) for name in ('frozen', 'no_grad')}
    assert torch.equal(params['frozen'].detach(), p0['frozen']) and torch.equal(params['no_grad'].detach(), p0['no_grad'])
    assert not opt.state[params['frozen']] and not opt.state[params['no_grad']]
    inside = torch.zeros_like(flat, dtype=torch.bool)
    for name in ('view9', 'view_two_chunks'):
        assert params[name].data_ptr() % 16 == 4
        start = (params[name].data_ptr() - flat.data_ptr()) // 4
        inside[start:start + params[name].numel()] = True
    assert bool((flat[~inside] == 7.0).all()) and int((~inside).sum()) >= 4
    for name in UPDATED:
        assert torch.equal(params[name].grad, values[name][1][STEPS - 1].to(DEV))


def test_two_runs_from_the_same_state_agree_to_the_bit(case):
    values = case[0]
    a, b = _hip_run(values), _hip_run(values)
    for key in ('p', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(_state(a[0], a[1], key), _state(b[0], b[1], key))
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def test_aligned_and_unaligned_paths_agree_to_the_bit(case):
    values = case[0]
    a, b = _hip_run(values), _hip_run(values, aligned_views=True)
    assert a[0]['view_two_chunks'].data_ptr() % 16 == 4 and b[0]['view_two_chunks'].data_ptr() % 16 == 0
    for key in ('p', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(_state(a[0], a[1], key), _state(b[0], b[1], key))
    # ... and with only the GRADIENT off the 16-byte grid (one of the four pointers is enough for the scalar path)
    params, _ = _params(values, DEV, torch.float32, aligned_views=True)
    opt = _hip_optimizer(params)
    for step in range(STEPS):
        _set_grads(params, values, step)
        for name in ('above', 'reg257'):
            g = params[name].grad
            shifted = torch.empty(g.numel() + 1, device=DEV)[1:].view_as(g).copy_(g)
            assert shifted.data_ptr() % 16 == 4
            params[name].grad = shifted
        opt.step()
    for key in ('p', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(_state(params, opt, key), _state(b[0], b[1], key))


def test_state_dict_moves_to_torch_adam(case):
    values, truth, want = case
    params, opt, _, _ = _hip_run(values, steps=2)
    theirs = torch.optim.Adam(list(params.values()), lr=LR, eps=EPS)
    theirs.load_state_dict(opt.state_dict())
    assert theirs.param_groups[0].keys() == torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).param_groups[0].keys()
    _set_grads(params, values, 2)
    _torch_step(params, theirs)                                        # the third step with torch's own operations, on the device
    _assert_all((params, theirs), want[:2], truth[:2], 'HIP, HIP, torch')


def test_state_dict_comes_from_torch_adam(case):
    values, truth, want = case
    params, theirs, _ = _torch_run(values, DEV, torch.float32, steps=2)
    opt = _hip_optimizer(params)
    assert opt.param_groups[0].keys() == theirs.param_groups[0].keys()
    opt.load_state_dict(theirs.state_dict())
    _set_grads(params, values, 2)
    opt.step()
    _assert_all((params, opt), want[:2], truth[:2], 'torch, torch, HIP')
    assert float(opt.state[params['above']]['step']) == 3


def test_exponential_lr_reaches_the_next_update():
    values = _values(1.0)
    truth = _torch_run(values, 'cpu', torch.float64, gamma=0.9)
    want = _torch_run(values, 'cpu', torch.float32, gamma=0.9)
    plain = _torch_run(values, 'cpu', torch.float64)
    params, opt, _, _ = _hip_run(values, gamma=0.9)
    assert opt.param_groups[0]['lr'] == pytest.approx(LR * 0.9 ** 3)
    _assert_all((params, opt), want[:2], truth[:2], 'ExponentialLR(0.9)')
    # the schedule is visible at this scale: the un-scheduled float64 run is far outside the rule
    moved = (_state(*plain[:2], 'p') - _state(*truth[:2], 'p')).abs().max()
    noise = (_state(*want[:2], 'p') - _state(*truth[:2], 'p')).abs().max()
    assert float(moved) > 10 * FACTORS[1] * float(noise)


def test_gradient_refusals_and_skipped_steps():
    values = _values(1.0)
    params, _ = _params(values, DEV, torch.float32)
    opt = _hip_optimizer(params)
    opt.step()                                                         # no gradient anywhere: nothing happens
    assert opt.last_grad_norm is None and not opt.state
    _set_grads(params, values, 0)
    params['seven'].grad = torch.zeros(7, 2, device=DEV)[:, 0]
    with pytest.raises(ValueError, match='the gradient of seven must be contiguous'):
        opt.step()
    params['seven'].grad = None
    params['three'].grad_dtype = None                                  # (torch itself refuses a float64 .grad on a float32 parameter otherwise)
    params['three'].grad = torch.zeros(3, device=DEV, dtype=torch.float64)
    with pytest.raises(ValueError, match=r'the gradient of three must be dense float32 \(got torch.float64'):
        opt.step()
    assert not any(float(s['step']) for s in opt.state.values())       # a refused step has counted nothing
    opt.param_groups[0]['weight_decay'] = 0.1
    with pytest.raises(ValueError, match='weight_decay=0.1 is not supported'):
        opt.step()


def test_model_step_matches_the_torch_recipe_and_invalidates_packed_weights():
    torch.manual_seed(3)
    model = nb.get_model(ARCH_A, use_rnn=True, dropout_rate=0.0, gpu=0).train()
    x = torch.randn(2, 80, 64, device=DEV)
    targets = torch.randint(1, 49, (2, 5), dtype=torch.int32, device=DEV)
    lengths = torch.full((2,), 5, dtype=torch.int32, device=DEV)
    out_len = torch.full((2,), 16, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        before = model.eval()(x).clone()
    session = model.stream(batch=2, max_chunk=64)
    session.push(x)
    session.reset()
    ctc.training_loss(model.train()(x), out_len, targets, lengths).backward()
    names = [name for name, _ in model.named_parameters()]
    assert all(p.grad is not None for p in model.parameters())

    conv = [i for i, p in enumerate(model.parameters())
            if any(p is m.conv.weight for m in model.modules() if isinstance(m, ops.PadConvRelu))]
    assert len(conv) == sum(isinstance(m, ops.PadConvRelu) for m in model.modules()) > 0

    def recipe(device, dtype):                                         # the reference's step with torch's operations on a deep copy
        twin = [p.detach().to(device=device, dtype=dtype).clone().requires_grad_() for p in model.parameters()]
        for p, q in zip(model.parameters(), twin):
            q.grad = p.grad.detach().to(device=device, dtype=dtype).clone()
        reg = 0.01 * sum(torch.norm(twin[i]) for i in conv)
        reg.backward()
        norm = torch.nn.utils.clip_grad_norm_(twin, 5)
        torch.optim.Adam(twin, lr=LR, eps=1e-7).step()
        return torch.cat([q.detach().reshape(-1).double().cpu() for q in twin]), float(norm)

    want, _ = recipe(DEV, torch.float32)
    truth, truth_norm = recipe('cpu', torch.float64)

    opt = optim.reference_optimizer(model, lr=LR)
    assert len(opt._weight_norm) == len(conv)
    opt.step()
    got = torch.cat([p.detach().reshape(-1).double().cpu() for p in model.parameters()])
    _assert_rule(got, want, truth, f'model step, {len(names)} tensors')
    assert abs(float(opt.last_grad_norm) - truth_norm) <= 2 * float(np.spacing(np.float32(truth_norm)))

    # the version bump reaches the packed-weight caches: the eval forward runs the STEPPED weights ...
    fresh = nb.get_model(ARCH_A, use_rnn=True, dropout_rate=0.0, gpu=0)
    fresh.load_state_dict(model.state_dict())
    with torch.no_grad():
        after, expected = model.eval()(x), fresh.eval()(x)
    assert torch.equal(after, expected) and not torch.equal(after, before)
    # ... and a streaming session that packed the old ones refuses to go on
    with pytest.raises(ValueError, match='create a new session'):
        session.push(x)
