"""nb_asr_amd.optim without a GPU: the chunk table, the argument checks of the C entry points, the refusals, the group layout."""
import pytest
import torch

from nb_asr_amd import hip, optim

CH = optim.CHUNK
SIZES = [1, 3, CH - 1, CH, CH + 1, 2 * CH + 5]


def _covered(counts, chunk):
    chunks, first, n = optim.chunk_table(counts, chunk)
    assert len(first) == len(n) == len(counts)
    at = 0
    for t, count in enumerate(counts):
        assert first[t] == at                                     # tensor by tensor, in table order
        own = chunks[first[t]:first[t] + n[t]]
        offset = 0
        for tensor, off, length in own:                          # ... every element once, ascending, no gap and no overlap
            assert tensor == t and off == offset and 1 <= length <= chunk and off % 4 == 0
            offset += length
        assert offset == count
        at += n[t]
    assert at == len(chunks)
    return chunks


@pytest.mark.parametrize('chunk', [CH, 8])
def test_chunk_table_covers_every_element_once_and_in_order(chunk):
    sizes = [1, 3, chunk - 1, chunk, chunk + 1, 2 * chunk + 5]
    chunks = _covered(sizes, chunk)
    assert [c[2] for c in chunks if c[0] == 5] == [chunk, chunk, 5]
    _covered(list(reversed(sizes)) + sizes, chunk)
    for size in sizes:
        _covered([size], chunk)


def test_chunk_table_of_no_tensors_and_of_empty_tensors():
    assert optim.chunk_table([]) == ([], [], [])
    assert optim.chunk_table([0, 5, 0], 4) == ([(1, 0, 4), (1, 4, 1)], [0, 0, 2], [0, 2, 0])
    assert CH % 4 == 0 and SIZES[-1] == 2 * CH + 5
    with pytest.raises(ValueError, match='multiple of 4'):
        optim.chunk_table([5], 6)
    with pytest.raises(ValueError, match='negative'):
        optim.chunk_table([-1])


def test_table_layout_matches_the_header():
    lib = hip.load_library()
    assert lib.nbasr_optim_table_bytes(3, 5) == 3 * optim.ROW_DTYPE.itemsize + 5 * optim.CHUNK_DTYPE.itemsize == 3 * 64 + 5 * 16
    assert lib.nbasr_optim_workspace_bytes(3, 5) == 5 * 3 * 8 + (3 + 1) * 4
    assert lib.nbasr_optim_table_bytes(0, 5) == 0 and lib.nbasr_optim_workspace_bytes(3, 0) == 0
    assert optim.ROW_DTYPE.names == ('p', 'grad', 'exp_avg', 'exp_avg_sq', 'count', 'flags', 'first_chunk', 'n_chunks', 'step_size', 'bc2_sqrt',
                                     'reserved')
    assert optim.CHUNK_DTYPE.names == ('tensor', 'length', 'offset')


def test_entry_point_argument_errors_are_reported_without_a_gpu():
    lib = hip.load_library()
    step = lib.nbasr_optim_adam_step
    # nbasr_optim_adam_step(table, n_tensors, n_chunks, workspace, total_norm, beta1, beta2, eps, max_norm, weight_norm_coef, stream)
    assert step(None, 1, 1, 16, 16, 0.9, 0.999, 1e-7, 5.0, 0.01, None) == -3 and b'non-NULL' in lib.nbasr_last_error()
    assert step(16, 1, 1, None, 16, 0.9, 0.999, 1e-7, 5.0, 0.01, None) == -3 and b'non-NULL' in lib.nbasr_last_error()
    assert step(16, 1, 1, 16, None, 0.9, 0.999, 1e-7, 5.0, 0.01, None) == -3 and b'non-NULL' in lib.nbasr_last_error()
    assert step(16, 0, 1, 16, 16, 0.9, 0.999, 1e-7, 5.0, 0.01, None) == -1 and b'positive' in lib.nbasr_last_error()
    assert step(16, 1, 0, 16, 16, 0.9, 0.999, 1e-7, 5.0, 0.01, None) == -1 and b'positive' in lib.nbasr_last_error()
    assert step(16, -2, -2, 16, 16, 0.9, 0.999, 1e-7, 5.0, 0.01, None) == -1 and b'positive' in lib.nbasr_last_error()
    assert step(16, 3, 2, 16, 16, 0.9, 0.999, 1e-7, 5.0, 0.01, None) == -1 and b'at least one chunk' in lib.nbasr_last_error()
    assert step(12, 1, 1, 16, 16, 0.9, 0.999, 1e-7, 5.0, 0.01, None) == -2 and b'8-byte aligned' in lib.nbasr_last_error()
    assert step(16, 1, 1, 16, 16, 1.0, 0.999, 1e-7, 5.0, 0.01, None) == -1 and b'beta1' in lib.nbasr_last_error()
    assert step(16, 1, 1, 16, 16, 0.9, 0.999, -1.0, 5.0, 0.01, None) == -1 and b'eps' in lib.nbasr_last_error()
    assert step(16, 1, 1, 16, 16, 0.9, 0.999, 1e-7, float('nan'), 0.01, None) == -1 and b'NaN' in lib.nbasr_last_error()


def test_cpu_parameters_are_refused():
    p = torch.nn.Parameter(torch.zeros(4, 3))
    with pytest.raises(ValueError, match=r'params\[0\] \(shape \(4, 3\)\) must be on a HIP device.*no CPU path'):
        optim.Adam([p])
    with pytest.raises(ValueError, match=r'w\.weight must be on a HIP device.*no CPU path'):
        optim.Adam([p], names={id(p): 'w.weight'})
    model = torch.nn.Linear(3, 2)
    with pytest.raises(ValueError, match=r'weight must be on a HIP device.*no CPU path'):
        optim.reference_optimizer(model)


def test_other_refusals():
    p = torch.nn.Parameter(torch.zeros(4, 3))
    with pytest.raises(ValueError, match=r'params\[0\] \(shape \(2,\)\) must be float32 \(got torch.float64\)'):
        optim.Adam([torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))])
    with pytest.raises(ValueError, match=r'params\[0\] \(shape \(3, 4\)\) must be dense and contiguous'):
        optim.Adam([torch.nn.Parameter(torch.zeros(4, 3).t())])
    with pytest.raises(ValueError, match=r'weight_norm_params\[0\] \(shape \(5,\)\) is not among params'):
        optim.Adam([p], weight_norm_coef=0.01, weight_norm_params=[torch.nn.Parameter(torch.zeros(5))])
    for option in ({'weight_decay': 0.1}, {'amsgrad': True}, {'maximize': True}):
        with pytest.raises(ValueError, match=f'{next(iter(option))}=.* is not supported'):
            optim.Adam([p], **option)
    with pytest.raises(ValueError, match='max_grad_norm'):
        optim.Adam([p], max_grad_norm=0.0)
    # gradients (checked in step(); the same checks on their own here, tests/test_optim_gpu.py has them through step())
    optim.check_companion(torch.zeros(4, 3), p, 'gradient', 'w')
    with pytest.raises(ValueError, match=r'the gradient of w must be dense float32 \(got torch.float16'):
        optim.check_companion(torch.zeros(4, 3, dtype=torch.float16), p, 'gradient', 'w')
    with pytest.raises(ValueError, match='the gradient of w must be contiguous'):
        optim.check_companion(torch.zeros(3, 4).t(), p, 'gradient', 'w')
    with pytest.raises(ValueError, match='the gradient of w must be dense float32'):
        optim.check_companion(torch.zeros(4, 3).to_sparse(), p, 'gradient', 'w')
    with pytest.raises(ValueError, match='device and shape'):
        optim.check_companion(torch.zeros(3, 4), p, 'exp_avg', 'w')


def test_group_keys_are_those_of_torch_adam():
    ours = optim.Adam.group_defaults(lr=1e-4, betas=(0.9, 0.999), eps=1e-7)
    theirs = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-4, eps=1e-7).param_groups[0]
    assert set(ours) | {'params'} == set(theirs)
    assert all(ours[k] == theirs[k] for k in ours)
    assert ours['eps'] == 1e-7 and ours['lr'] == 1e-4


def test_bias_corrections_are_torchs():
    step_size, bc2_sqrt = optim.bias_corrections(1e-4, 0.9, 0.999, 3)
    assert step_size == 1e-4 / (1 - 0.9 ** 3) and bc2_sqrt == (1 - 0.999 ** 3) ** 0.5
