"""The drop-in boundary as code: ``nb_asr_amd.register_with(nasbench_asr)`` makes this package the reference's
'hip' model backend with no edit to the reference (model/__init__.py:4,19-24; utils.py:150-153).  What the reference itself returned
once registered -- and its torch backend's state_dict layout -- is recorded in tests/golden/reference_answers.json
(tests/golden/make_reference_answers.py ran the reference); here the registration is made into a stand-in holding the two
attributes of the reference's backend accessor that it seeds, and the entry points it hands over are held to those answers."""
import json
import pathlib
import types

import pytest
import torch

import nb_asr_amd

ANSWERS = json.loads((pathlib.Path(__file__).resolve().parent / 'golden' / 'reference_answers.json').read_text())['registration']
ARCH = [[3, 1], [4, 1, 1], [2, 1, 1, 1]]


@pytest.fixture()
def nasbench_asr():
    """The attributes register_with touches: model._backends.backends (name -> backend module) and .available_backends."""
    accessor = types.SimpleNamespace(backends={}, available_backends=['torch'])
    return types.SimpleNamespace(model=types.SimpleNamespace(_backends=accessor))


def _type_name(model):
    return f'{type(model).__module__}.{type(model).__qualname__}'


def test_reference_get_model_returns_the_hip_model(nasbench_asr, capsys):
    assert ANSWERS['arch'] == ARCH
    assert nb_asr_amd.register_with(nasbench_asr) == 'hip'
    accessor = nasbench_asr.model._backends
    assert accessor.backends == {'hip': nb_asr_amd} and accessor.available_backends == ['torch', 'hip']
    want = ANSWERS['hip']
    assert want['hip_available'] is True
    # the reference's get_model(..., backend='hip') resolves 'hip' through that dict and calls the module's get_model (model/__init__.py:19-20)
    model = accessor.backends['hip'].get_model(ARCH, use_rnn=True, dropout_rate=0.0)
    assert isinstance(model, nb_asr_amd.model.ASRModel) and _type_name(model) == want['type']
    assert model.backend == want['backend_attr'] == 'hip' and model.training is want['training'] is True
    assert sum(p.numel() for p in model.parameters()) == want['parameters'] == 27032549
    # same state_dict keys and shapes as the reference's torch backend: checkpoints move between the two unchanged
    assert ANSWERS['torch_backend_type_module'].startswith('nasbench_asr.')
    theirs_shapes = ANSWERS['torch_backend_state_dict_shapes']
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == theirs_shapes
    gen = torch.Generator().manual_seed(0)
    theirs = {k: torch.randn(shape, generator=gen) for k, shape in theirs_shapes.items()}
    model.load_state_dict(theirs)
    assert all(torch.equal(v, theirs[k]) for k, v in model.state_dict().items())
    # print_model_summary dispatches on model.backend (model/__init__.py:23-24) back into this package
    accessor.backends[model.backend].print_model_summary(model)
    out = capsys.readouterr().out
    assert 'Trainable parameters: 27,032,549' in out
    # the torch backend is untouched and still the default
    assert 'torch' not in accessor.backends and None not in accessor.backends


def test_register_as_default_backend(nasbench_asr):
    nb_asr_amd.register_with(nasbench_asr, default=True)
    accessor = nasbench_asr.model._backends
    assert accessor.backends[None] is nb_asr_amd and accessor.backends['hip'] is nb_asr_amd
    model = accessor.backends[None].get_model(ARCH, use_rnn=False, dropout_rate=0.0)                    # get_model(...) without backend=
    want = ANSWERS['default_no_rnn']
    assert isinstance(model, nb_asr_amd.model.ASRModel) and _type_name(model) == want['type']
    assert sum(p.numel() for p in model.parameters()) == want['parameters'] == 23662849 and model.use_rnn is want['use_rnn'] is False


def test_no_cpu_forward_through_the_reference_entry_point(nasbench_asr):
    """The registered backend keeps the package's contract: a CPU tensor raises, nothing falls back to torch."""
    nb_asr_amd.register_with(nasbench_asr)
    model = nasbench_asr.model._backends.backends['hip'].get_model(ARCH, use_rnn=True, dropout_rate=0.0).eval()
    with pytest.raises(nb_asr_amd.hip.HipError):
        model(torch.zeros(1, 80, 16))
