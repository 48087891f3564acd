"""The package ``nb_asr_amd.ctc`` keeps the surface the one-file module had (tests/golden/ctc_surface.json, recorded from it: every top-level
name, the signature of every callable, of every class the signatures of ``__init__`` and the public methods, the value of every constant),
each name has one home, the families import along one graph, and the three record views read their record as views (no GPU needed).

The record was made from the one-file module by::

    def members(cls):      # the public methods, properties and __init__ that the package's own classes give ``cls``
        found = {}
        for klass in reversed(cls.__mro__):
            if klass.__module__.startswith('nb_asr_amd'):
                for name, v in vars(klass).items():
                    if name == '__init__' or not name.startswith('_'):
                        found[name] = ('property' if isinstance(v, property) else
                                       str(inspect.signature(getattr(cls, name))) if callable(getattr(cls, name)) else None)
        return {name: v for name, v in found.items() if v}

    names = {n: v for n, v in vars(ctc).items() if not n.startswith('__')}
    modules = sorted(n for n, v in names.items() if isinstance(v, types.ModuleType))
    names = {n: v for n, v in sorted(names.items()) if n not in modules}
    json.dump({'modules': modules, 'names': list(names),
               'callables': {n: str(inspect.signature(v)) for n, v in names.items() if callable(v)},
               'methods': {n: members(v) for n, v in names.items() if inspect.isclass(v)},
               'constants': {n: v for n, v in names.items() if isinstance(v, (int, float, str, tuple))}}, file, indent=1, sort_keys=True)
"""
import ast
import inspect
import json
import pathlib
import types

import pytest
import torch

from nb_asr_amd import ctc, hip

SURFACE = json.loads((pathlib.Path(__file__).parent / 'golden' / 'ctc_surface.json').read_text())
PACKAGE = sorted(pathlib.Path(ctc.__file__).parent.glob('*.py'))
# who a family may import from inside the package ('' is the core); outside it, the binding and the phoneme tables only
IMPORTS = {'decode': {''}, 'detect': {''}, 'score': {'', 'decode'}, 'record_detectors': {'', 'detect'}, 'token_confidence': {'', 'detect', 'score'}}


def _members(cls):
    return {name: 'property' if isinstance(inspect.getattr_static(cls, name), property) else str(inspect.signature(getattr(cls, name)))
            for name in SURFACE['methods'][cls.__name__]}


def _plain(value):
    return list(value) if isinstance(value, tuple) else value


def test_every_name_is_there_with_its_signature_or_value():
    # 73 = the 69 names recorded + the 4 modules the one-file module imported (collections, hip, inspect, torch), which count among its 53 public names
    assert len(SURFACE['names']) + len(SURFACE['modules']) == 73 and len(SURFACE['callables']) == 57 and len(SURFACE['methods']) == 19
    assert sum(not n.startswith('_') for n in SURFACE['names'] + SURFACE['modules']) == 53 and len(SURFACE['constants']) == 11
    assert [n for n in SURFACE['names'] if not hasattr(ctc, n)] == []
    assert [n for n in SURFACE['modules'] if not isinstance(getattr(ctc, n, None), types.ModuleType)] == []
    assert {n: str(inspect.signature(getattr(ctc, n))) for n in SURFACE['callables']} == SURFACE['callables']
    assert {n: _members(getattr(ctc, n)) for n in SURFACE['methods']} == SURFACE['methods']
    assert {n: _plain(getattr(ctc, n)) for n in SURFACE['constants']} == SURFACE['constants']
    assert {n: type(getattr(ctc, n)).__name__ for n in SURFACE['constants']} == {n: type(v).__name__.replace('list', 'tuple') for n, v in SURFACE['constants'].items()}
    assert ctc.hip is hip and ctc.fold_table.__module__ == 'nb_asr_amd.phonemes'
    for name in SURFACE['callables']:                        # docstrings travel with their code
        if name not in ('Alignment', '_TrainingLoss', '_lengths', '_positive', '_segment_rules', '_confidence_rules'):
            assert len(getattr(ctc, name).__doc__ or '') > 40, name


def test_one_definition_per_name_and_one_way_imports():
    assert [p.stem for p in PACKAGE] == ['__init__'] + sorted(IMPORTS)
    defined = {}
    for path in PACKAGE:
        tree = ast.parse(path.read_text())
        for node in tree.body:
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
                defined.setdefault(node.name, []).append(path.name)
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                assert not any(alias.name.startswith('nb_asr_amd') for alias in node.names), path.name
            if not isinstance(node, ast.ImportFrom) or not node.level:
                assert not (isinstance(node, ast.ImportFrom) and node.module.startswith('nb_asr_amd')), path.name
                continue
            if path.stem == '__init__':                      # the core: the binding, the front-end's constants, the label table; then its families
                assert (node.level, node.module) in [(2, None), (2, 'frontend'), (2, 'phonemes')] or (node.level == 1 and node.module in IMPORTS)
            elif node.level == 1:
                assert (node.module or '') in IMPORTS[path.stem], (path.name, node.module)
                if node.module is None:                      # from the core, never a sibling by way of the package
                    assert not {alias.name for alias in node.names} & set(IMPORTS), path.name
            else:
                assert (node.level, node.module) == (2, 'phonemes'), (path.name, node.module)
    assert {name: files for name, files in defined.items() if len(files) > 1} == {}
    assert set(SURFACE['methods']) | {n for n in SURFACE['callables']} <= set(defined) | {'fold_table', 'LogMelFrontend', 'Alignment'}
    lines = [len(path.read_text().splitlines()) for path in PACKAGE]
    assert max(lines) <= 450 and sum(lines) <= 1461                  # no file too long, and all of them no longer than the one file was


def test_a_class_exists_once_whichever_way_it_is_reached():
    for name in SURFACE['names']:
        homes = [m for m in IMPORTS if name in vars(getattr(ctc, m))]
        assert all(getattr(getattr(ctc, m), name) is getattr(ctc, name) for m in homes), name
    assert all(isinstance(getattr(ctc, m), types.ModuleType) for m in IMPORTS)              # no family shares a name with what it defines
    assert ctc._LogitDetectorStream is ctc.detect._LogitDetectorStream and ctc.detect._chunk_rows is ctc._chunk_rows
    for stream, result, whole, home in ((ctc.EndpointStream, ctc.EndpointResult, ctc.endpoint, ctc.record_detectors),
                                        (ctc.SegmentStream, ctc.SegmentResult, ctc.segment, ctc.record_detectors),
                                        (ctc.KeywordStream, ctc.KeywordResult, ctc.spot_keywords, ctc.record_detectors),
                                        (ctc.ConfidenceStream, ctc.ConfidenceResult, ctc.confidence, ctc.token_confidence)):
        assert stream.RESULT is result and issubclass(stream, ctc.detect._LogitDetectorStream)
        assert stream.__module__ == result.__module__ == whole.__module__ == home.__name__
    assert ctc.score.beam_decode is ctc.decode.beam_decode is ctc.beam_decode and ctc.token_confidence.forced_align is ctc.forced_align
    assert issubclass(ctc.SegmentRules, ctc._SpeechDecision) and issubclass(ctc.EndpointRules, ctc.detect._SpeechDecision)
    assert ctc._segment_rules(None).counts == ctc.SegmentRules().counts and ctc._confidence_rules(None).measure == 'tsallis'


RECORDS = [(ctc.EndpointResult, lambda: ctc._fresh_endpoint_state(3)), (ctc.SegmentResult, lambda: ctc._fresh_segment_state(3, 2)),
           (ctc.KeywordResult, lambda: ctc._fresh_keyword_state(3, 2))]


@pytest.mark.parametrize('cls,fresh', RECORDS, ids=[cls.__name__ for cls, _ in RECORDS])
def test_a_record_view_shows_its_record_as_views(cls, fresh):
    state = fresh()
    state.view(-1)[:] = torch.arange(state.numel(), dtype=torch.int32)       # every word differs
    r = cls(state)
    first, last = state.data_ptr(), state.data_ptr() + state.numel() * 4
    assert r.state is state and state.dtype == torch.int32
    for name in cls.FIELDS:
        field = getattr(r, name)
        assert field.dtype == (torch.float32 if cls is ctc.KeywordResult and name.endswith('_score') else torch.int32), name
        assert field.shape == state.shape[:-1] and first <= field.data_ptr() < last, name
        word = (field.data_ptr() - first) // 4
        assert torch.equal(field.view(torch.int32), state[..., word]) and word == cls.FIELDS.index(name), name
    assert first <= r.frames.data_ptr() < last
    state[..., 0] += 7                                                       # a view moves with its record
    assert torch.equal(r.frames, state[..., 0])
    kept = r.clone()
    assert type(kept) is cls and torch.equal(kept.state, state) and kept.state.data_ptr() != first
    state[..., 0] += 1
    assert not torch.equal(kept.frames, r.frames)
    assert repr(r).startswith(cls.__name__ + '(frames=') and all(f'{name}=' in repr(r) for name in cls.FIELDS)
    assert all(t.dtype == torch.float32 for t in r.seconds())
    if cls is ctc.SegmentResult:
        assert r.capacity == 2 and r.ring.shape == (3, 2, 4) and first <= r.ring.data_ptr() < last and r.dropped.shape == (3,)
    if cls is ctc.KeywordResult:
        assert r.detected.dtype == torch.bool and r.detected.shape == (3, 2)


def test_frame_seconds_is_the_one_conversion():
    frames = torch.tensor([-1, 0, 3, 25], dtype=torch.int32)
    want = torch.tensor([-1.0, 0.0, 3 * ctc.FRAME_SECONDS, 25 * ctc.FRAME_SECONDS])
    assert torch.equal(ctc.EndpointResult._frame_seconds(frames), want)
    state = ctc._fresh_endpoint_state(4)
    state[:, 4] = frames
    assert torch.equal(ctc.EndpointResult(state).seconds()[0], want) and torch.equal(ctc.EndpointResult(state).seconds()[1], torch.full((4,), -1.0))
    record = ctc._fresh_keyword_state(1, 1)
    record[0, 0, 1], record[0, 0, 2] = 9, 4                                  # a hit that started at frame 4 and ended with frame 9
    hit_start, hit_end, best_start, best_end = ctc.KeywordResult(record).seconds()
    assert hit_start.item() == pytest.approx(4 * ctc.FRAME_SECONDS) and hit_end.item() == pytest.approx(10 * ctc.FRAME_SECONDS)
    assert best_start.item() == best_end.item() == -1.0
