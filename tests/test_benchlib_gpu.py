"""tools/benchlib.py and tools/bench_detector.py on the device: the plumbing at its smallest shape, not the kernels' speed."""
import json
import math
import pathlib
import sys

import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent / 'tools'))

import benchlib                                  # noqa: E402
import bench_detector                            # noqa: E402


@pytest.mark.gpu
def test_window_and_the_segment_tool_on_the_device(tmp_path):
    x, calls = torch.zeros(8, device='cuda:0'), []
    ms = benchlib.window(lambda: calls.append(x.add_(1)), calls=3)
    assert len(calls) == 3 and x.tolist() == [3.0] * 8 and math.isfinite(ms) and ms > 0
    out = tmp_path / 'segment.json'
    rows = bench_detector.main(['--detector', 'segment', '--pushes', '2', '--reps', '2', '--batches', '1', '--out', str(out)])
    steps = [kind for _ in (1, 10, 40) for kind in ('EndpointStream.push', 'SegmentStream.push', 'SegmentStream.push over EndpointStream.push')]
    assert [r['what'] for r in rows] == ['StreamingSession.push', 'StreamingSession.push', 'added by segments=', 'ctc.segment'] + steps
    assert [r.get('session') for r in rows[:2]] == ['without segments=', 'with segments='] and all(r['batch'] == 1 for r in rows if 'batch' in r)
    assert [r['frames'] for r in rows[4:]] == [n for n in (1, 10, 40) for _ in range(3)]
    assert list(rows[0]) == ['what', 'session', 'library', 'batch', 'frames_per_push', 'us', 'us_min', 'us_max']
    assert list(rows[3]) == ['what', 'shape', 'us', 'us_min', 'us_max', 'bytes', 'gb_per_s'] and rows[3]['shape'] == [64, 250, 49]
    assert all(r['us_min'] <= r['us'] <= r['us_max'] and r['us_min'] > 0 for r in rows if 'us_min' in r)
    assert all(math.isfinite(r['ratio']) and r['ratio'] > 0 for r in rows if 'ratio' in r)
    assert json.loads(out.read_text()) == rows
