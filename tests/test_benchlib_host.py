"""tools/benchlib.py and tools/bench_detector.py without a GPU: who is called when (the window is a fake that records its calls and returns
scripted times), what a summary holds, how a child's output becomes the parent's rows, the ratio rows from a hand-written list, and the
per-detector table."""
import inspect
import json
import pathlib
import sys
import types

import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent / 'tools'))

import benchlib                                  # noqa: E402
import bench_detector                            # noqa: E402
from nb_asr_amd import ctc, streaming            # noqa: E402


@pytest.fixture
def events(monkeypatch):
    """What happened, in order: ('call', name) by the functions below, ('window', name, calls) by the fake window, 'sync'."""
    log = []
    monkeypatch.setattr(benchlib.torch.cuda, 'synchronize', lambda: log.append('sync'))
    return log


def functions(events, names):
    def make(name):
        fn = lambda: events.append(('call', name))      # noqa: E731
        fn.name = name
        return fn
    return [make(name) for name in names]


def test_alternate_takes_turns_after_the_warm_up(events):
    script = iter(range(100))

    def window(fn, calls):
        events.append(('window', fn.name, calls))
        return float(next(script))

    times = benchlib.alternate(functions(events, 'ab'), calls=5, reps=3, warmup=2, window=window)
    assert events == [('call', 'a')] * 2 + [('call', 'b')] * 2 + ['sync'] + [('window', 'a', 5), ('window', 'b', 5)] * 3
    assert times == [[0.0, 2.0, 4.0], [1.0, 3.0, 5.0]]                  # raw, per function, in the order measured


def test_alternate_without_warm_up_calls_nothing_first(events):
    times = benchlib.alternate(functions(events, 'abc'), reps=2, window=lambda fn, calls: events.append((fn.name, calls)) or 1.5)
    assert events == [('a', 1), ('b', 1), ('c', 1)] * 2 and times == [[1.5, 1.5]] * 3


def test_warm_calls_each_function_n_times_then_waits(events):
    benchlib.warm(functions(events, 'ab'), 3)
    assert events == [('call', 'a')] * 3 + [('call', 'b')] * 3 + ['sync']


def test_window_is_the_default_of_alternate():
    assert inspect.signature(benchlib.alternate).parameters['window'].default is benchlib.window
    assert [p.default for p in list(inspect.signature(benchlib.alternate).parameters.values())[1:4]] == [1, 7, 0]


def test_summary():
    times = [0.0123456, 0.0100004, 0.0149996, 0.02]                     # ms: median 0.0136726
    assert benchlib.summary(times) == (pytest.approx(0.0136726, rel=1e-12), 0.0100004, 0.02)
    assert benchlib.summary(times, 'us', scale=1e3) == {'us': 13.67, 'us_min': 10.0, 'us_max': 20.0}
    assert benchlib.summary(times, 'ms', digits=4) == {'ms': 0.0137, 'ms_min': 0.01, 'ms_max': 0.02}
    assert list(benchlib.summary([3.0], 'us')) == ['us', 'us_min', 'us_max']


def test_child_rows_keeps_the_json_lines_and_names_the_parent():
    stdout = 'warning: something\n{"what": "StreamingSession.push", "library": "/tmp/old.so", "batch": 1, "us": 2.5}\n\n  {"indented": 1}\n' \
             '{"what": "StreamingSession.push", "library": "/tmp/old.so", "batch": 16, "us": 3.5}\nbye\n'
    before, after = benchlib.child_rows(stdout, 'before'), benchlib.child_rows(stdout, 'after')
    assert [(r['batch'], r['us']) for r in before] == [(1, 2.5), (16, 3.5)]
    assert {r['library'] for r in before} == {'parent (before this one)'} and {r['library'] for r in after} == {'parent (after this one)'}


def test_parent_rows_start_a_fresh_child_process(monkeypatch, capsys):
    seen = {}

    def run(cmd, **kw):
        seen.update(cmd=cmd, kw=kw)
        return types.SimpleNamespace(returncode=0, stdout='{"library": "x", "batch": 1, "us": 1.0}\n', stderr='')
    monkeypatch.setattr(benchlib.subprocess, 'run', run)
    rows = benchlib.parent_rows('tools/bench_detector.py', '/tmp/old.so', 'after', ['--pushes', '3'])
    assert seen['cmd'][0] == sys.executable and pathlib.Path(seen['cmd'][1]).name == 'bench_detector.py'
    assert seen['cmd'][2:] == ['--library', '/tmp/old.so', '--pushes', '3'] and seen['kw']['timeout'] == 300
    assert rows == [{'library': 'parent (after this one)', 'batch': 1, 'us': 1.0}]
    assert json.loads(capsys.readouterr().out) == rows[0]              # a row is printed as soon as it exists
    monkeypatch.setattr(benchlib.subprocess, 'run', lambda cmd, **kw: types.SimpleNamespace(returncode=1, stdout='', stderr='boom'))
    with pytest.raises(SystemExit, match='boom'):
        benchlib.parent_rows('tools/bench_detector.py', '/tmp/old.so', 'before', [])


def test_parent_ratio_rows():
    def push(library, session, batch, us):
        return {'what': 'StreamingSession.push', 'session': session, 'library': library, 'batch': batch, 'frames_per_push': 40, 'us': us}
    rows = [push('parent (before this one)', 'without segments=', 1, 1000.0), push('parent (before this one)', 'without segments=', 16, 2000.0),
            push('this', 'without segments=', 1, 1010.0), push('this', 'with segments=', 1, 5000.0),
            {'what': 'added by segments=', 'library': 'this', 'batch': 1, 'us': 3990.0, 'ratio': 4.9505},
            push('this', 'without segments=', 16, 1990.0), push('this', 'with segments=', 16, 6000.0),
            push('parent (after this one)', 'without segments=', 1, 1020.0), push('parent (after this one)', 'without segments=', 16, 1980.0)]
    assert benchlib.parent_ratio_rows(rows, [1, 16], 'without segments=') == [
        {'what': 'plain push, this library over the parent\'s', 'batch': 1, 'parent_us': 1010.0, 'ratio': 1.0, 'parent_legs_ratio': 1.02},
        {'what': 'plain push, this library over the parent\'s', 'batch': 16, 'parent_us': 1990.0, 'ratio': 1.0, 'parent_legs_ratio': 1.0101}]
    rows[2]['us'] = 1015.05
    assert benchlib.parent_ratio_rows(rows, [1], 'without segments=')[0]['ratio'] == 1.005


def test_emit_and_write_out(tmp_path, capsys):
    rows = []
    assert benchlib.emit(rows, {'a': 1}) is rows[0]
    assert capsys.readouterr().out == '{"a": 1}\n'
    benchlib.write_out(None, rows)
    benchlib.write_out(str(tmp_path / 'deep' / 'out.json'), rows)
    assert json.loads((tmp_path / 'deep' / 'out.json').read_text()) == [{'a': 1}]


def test_no_device_is_an_error(monkeypatch):
    monkeypatch.setattr(benchlib.torch.cuda, 'is_available', lambda: False)
    with pytest.raises(SystemExit, match='needs a HIP device'):
        benchlib.need_device('bench_detector.py')
    with pytest.raises(SystemExit, match='needs a HIP device'):
        bench_detector.main(['--detector', 'segment'])


def test_detector_table():
    assert sorted(bench_detector.DETECTORS) == ['endpoint', 'keyword', 'segment']
    specs = {'endpoint': ctc.EndpointRules, 'keyword': ctc.KeywordSet, 'segment': ctc.SegmentRules}
    streams = {'endpoint': ctc.EndpointStream, 'keyword': ctc.KeywordStream, 'segment': ctc.SegmentStream}
    session = inspect.signature(streaming.StreamingSession.__init__).parameters
    for name, det in bench_detector.DETECTORS.items():
        assert isinstance(det['spec'](None), specs[name]) and det['stream'] is streams[name] and det['kwarg'] in session
        for extra, spec, frames in det['grid']:
            assert isinstance(spec(None), specs[name]) and all(n >= 1 for n in frames)
    endpoint, keyword, segment = (bench_detector.DETECTORS[k] for k in ('endpoint', 'keyword', 'segment'))
    assert [g[2] for g in endpoint['grid']] == [(1, 10, 40)] == [g[2] for g in segment['grid']]
    assert [(g[0], g[2]) for g in keyword['grid']] == [({'keywords': n}, (4, 250)) for n in (1, 8, 64)]
    assert [len(g[1](None).keywords) for g in keyword['grid']] == [1, 8, 64] and len(keyword['spec'](None).keywords) == 8
    assert (endpoint['whole'], keyword['whole'], segment['whole']) == (ctc.endpoint, None, ctc.segment)
    assert (endpoint['beside'], keyword['beside'], segment['beside']) == (None, None, 'endpoint')
    assert keyword['added'] == {'keywords': 8} and endpoint['added'] == {} == segment['added']
