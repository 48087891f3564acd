"""The binding package ``nb_asr_amd.hip`` keeps the surface the one-file binding had (tests/golden/hip_surface.json, recorded from it: every
top-level name, the signature of every callable, the value of every constant, the beam table; one entry differs from the record, the
private ``_beam_call``, whose leading library argument went when ``_call`` began to find the library), keeps its state in the package's own module
where the tools and tests outside write to it, and its three shared helpers -- ``_call``, ``_scratch``, ``_opaque`` -- do what every
wrapper relies on (no GPU needed)."""
import ast
import inspect
import json
import pathlib

import pytest
import torch

from nb_asr_amd import build, hip

SURFACE = json.loads((pathlib.Path(__file__).parent / 'golden' / 'hip_surface.json').read_text())
PACKAGE = sorted(pathlib.Path(hip.__file__).parent.glob('*.py'))


def _signature(value):
    try:
        return str(inspect.signature(value))
    except (ValueError, TypeError):          # the ctypes aliases
        return None


def test_every_name_is_there_with_its_signature_or_value():
    assert len(SURFACE['names']) == 170 and len(SURFACE['callables']) == 142
    assert [n for n in SURFACE['names'] if not hasattr(hip, n)] == []
    assert {n: _signature(getattr(hip, n)) for n in SURFACE['callables']} == SURFACE['callables']
    assert {n: getattr(hip, n) for n in SURFACE['constants']} == SURFACE['constants']
    for name in ('pack_pointwise_weights', 'pointwise_bf16_workspace', 'linear_fused_packed', 'linear_fused_bf16'):      # bound bodies keep words
        assert 'partial(' not in getattr(hip, name).__doc__ and len(getattr(hip, name).__doc__) > 40, name
    assert {f'{op},{int(timed)},{int(fused)}': [name, args] for (op, timed, fused), (name, args) in hip.BEAM_ENTRY_POINTS.items()} \
        == SURFACE['beam_entry_points']


def test_the_state_lives_in_the_package_module(monkeypatch, tmp_path):
    assert hip.LIB_PATH == build.LIB_PATH
    # SIGNATURES is the table load_library reads: a deleted entry is left untyped (benchlib.bind_library relies on it)
    saved = hip.SIGNATURES.pop('nbasr_convert')
    try:
        lib = hip.load_library(hip.LIB_PATH)
        assert lib.nbasr_convert.argtypes is None and lib.nbasr_repitch.argtypes == hip.SIGNATURES['nbasr_repitch'][1]
    finally:
        hip.SIGNATURES['nbasr_convert'] = saved
    assert hip.load_library(hip.LIB_PATH).nbasr_convert.argtypes == saved[1]
    # LIB_PATH is the path load_library opens
    monkeypatch.setattr(hip, '_lib', None)
    monkeypatch.setattr(hip, 'LIB_PATH', tmp_path / 'libnbasr_hip.so')
    with pytest.raises(hip.HipError, match='has not been built'):
        hip.load_library()


def test_one_definition_per_name_and_one_home_for_the_state():
    assert len(PACKAGE) == 7 and hip.__file__ == str(PACKAGE[0])
    defined, state = {}, set()
    for path in PACKAGE:
        tree = ast.parse(path.read_text())
        for node in tree.body:
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
                defined.setdefault(node.name, []).append(path.name)
        for node in ast.walk(tree):
            if isinstance(node, ast.Name) and isinstance(node.ctx, ast.Store) and node.id in ('_lib', '_tls'):
                state.add(path.name)
            if isinstance(node, ast.ImportFrom) and node.level and path.name != '__init__.py':
                assert node.level == 1 and node.module is None, (path.name, node.module)       # a family imports from the core only
    assert {name: files for name, files in defined.items() if len(files) > 1} == {}
    assert state == {'__init__.py'}
    # the taped set is drawn from the whole table, after the families registered theirs
    assert hip._ENQUEUES == {n for n in hip.SIGNATURES if n not in hip._HOST_ONLY and not n.endswith('_bytes') and '_bytes_' not in n}
    assert {'nbasr_lstm_backward_step', 'nbasr_ctc_keyword_step', 'nbasr_resample', 'nbasr_pad_amounts'} - hip._ENQUEUES == {'nbasr_pad_amounts'}


@pytest.mark.parametrize('dtype', [torch.uint8, torch.int32, torch.float32, torch.int64])
def test_scratch_covers_the_bytes_asked_for(dtype):
    """3 076 is the workspace that lost its last 4 bytes to ``// 8``."""
    for nbytes in (0, 1, 3, 4, 7, 8, 3076, 3077):
        t = hip._scratch(nbytes, 'cpu', dtype)
        have = t.numel() * t.element_size()
        assert t.dtype == dtype and t.dim() == 1 and t.data_ptr() != 0
        assert max(nbytes, 8) <= have < max(nbytes, 8) + dtype.itemsize, (nbytes, have)
    assert hip._scratch(3, 'cpu', least=16).numel() == 16 and hip._scratch(0, 'cpu', torch.float32, 0).numel() == 1


class _Image:
    """As much of a device tensor as ``_opaque`` looks at."""
    is_cuda = True

    def __init__(self, nbytes, dtype=torch.uint8, contiguous=True, device='cuda:0'):
        self._n, self.dtype, self._contiguous, self.device = nbytes // dtype.itemsize, dtype, contiguous, device

    def numel(self):
        return self._n

    def element_size(self):
        return self.dtype.itemsize

    def is_contiguous(self):
        return self._contiguous


def test_opaque_is_the_size_check_with_the_callers_words():
    image = _Image(96)
    assert hip._opaque(image, 96, 'm') is image and hip._opaque(image, 96, 'm', exact=True) is image and hip._opaque(_Image(97), 96, 'm')
    for bad, kwargs in ((_Image(95), {}), (_Image(95), {'exact': True}), (_Image(97), {'exact': True}), (_Image(96, contiguous=False), {}),
                        (_Image(96, torch.int32), {}), (_Image(96), {'device': 'cuda:1'}), (torch.empty(96, dtype=torch.uint8), {}), (None, {})):
        with pytest.raises(hip.HipError) as err:
            hip._opaque(bad, 96, 'packed weights are not what pack_x made', **kwargs)
        assert str(err.value) == 'packed weights are not what pack_x made' and err.value.code is None
    with pytest.raises(hip.HipError, match='^ws of 96 bytes from pointwise_workspace$'):             # (format, *values): formatted on failure only
        hip._opaque(_Image(95), 96, ('ws of {} bytes from {}', 96, 'pointwise_workspace'))
    assert hip._opaque(_Image(96, torch.int32), 96, 'm', dtype=None, device='cuda:0')       # a state: any dtype, on the chunk's device


class _Library:
    """Two entry points that answer on the host: they return their first argument and keep the rest."""

    def __init__(self):
        self.seen = []

    def nbasr_channel_stats(self, rc, *args):
        self.seen.append(args)
        return rc

    def nbasr_split_image_bytes(self, rc, *args):
        self.seen.append(args)
        return rc

    def nbasr_last_error(self):
        return b'said the library'


def test_call_names_the_entry_point_once_and_goes_through_the_tape(monkeypatch):
    lib = _Library()
    monkeypatch.setattr(hip, '_lib', lib)
    assert hip._call('nbasr_channel_stats', 0, 1, None, 2.5) is None and lib.seen == [(1, None, 2.5)]
    with pytest.raises(hip.HipError, match='nbasr_channel_stats failed with code -2: said the library') as err:
        hip._call('nbasr_channel_stats', -2, 7)
    assert err.value.code == -2
    entries = []
    hip.start_tape(entries)
    try:
        hip._call('nbasr_channel_stats', 0, 5, 6)
        hip._call('nbasr_split_image_bytes', 0, 5)            # a query: executed, not recorded
    finally:
        hip.stop_tape()
    assert len(entries) == 1 and entries[0][1] == [0, 5, 6] and entries[0][0].__name__ == 'nbasr_channel_stats'
    assert entries[0][0].__self__ is lib and lib.seen[-2:] == [(5, 6), (5,)]
    # _check is read from the package at call time (tests/test_executor_host.py patches it)
    monkeypatch.setattr(hip, '_check', lambda rc, what: lib.seen.append((rc, what)))
    hip._call('nbasr_channel_stats', 9)
    assert lib.seen[-1] == (9, 'nbasr_channel_stats')
