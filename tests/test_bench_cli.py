"""bench.py's own contract: a plain run times the headline leg and prints the contract fields; `--dump-outputs DIR` writes the logits
of the last timed step (float32, at most 64 MB: a seeded sample of whole utterances above that)."""
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import bench  # noqa: E402


def test_dump_outputs_writes_the_logits_as_float32(tmp_path):
    logits = torch.randn(4, 25, 49, dtype=torch.float64).to(torch.bfloat16)
    (tmp_path / 'logits_rows.npy').write_bytes(b'stale')
    bench.dump_outputs(str(tmp_path), logits)
    got = np.load(tmp_path / 'logits.npy')
    assert got.dtype == np.float32 and got.shape == (4, 25, 49)
    assert np.array_equal(got, logits.float().numpy())
    assert not (tmp_path / 'logits_rows.npy').exists()


def test_dump_outputs_samples_whole_utterances_above_the_limit(tmp_path):
    rows, frames = 300, 1200                                  # 300 x 1200 x 49 x 4 B = 70.6 MB
    logits = torch.arange(rows, dtype=torch.float32).view(rows, 1, 1).expand(rows, frames, 49).contiguous()
    for run in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / run), logits)
    total = sum(f.stat().st_size for f in (tmp_path / 'a').iterdir())
    assert total <= bench.DUMP_LIMIT_BYTES
    got, idx = np.load(tmp_path / 'a' / 'logits.npy'), np.load(tmp_path / 'a' / 'logits_rows.npy')
    assert got.dtype == np.float32 and idx.dtype == np.float64 and got.shape[1:] == (frames, 49)
    assert 0 < got.shape[0] < rows and got.shape[0] == idx.shape[0] and np.all(np.diff(idx) > 0)
    assert np.array_equal(got[:, 0, 0], idx.astype(np.float32))          # whole utterances, the ones named by the indices
    assert np.array_equal(idx, np.load(tmp_path / 'b' / 'logits_rows.npy'))          # a fixed sample


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_logits(tmp_path):
    out = subprocess.run([sys.executable, str(REPO / 'bench.py'), '--gpus', '1', '--batch', '8', '--frames', '200', '--steps', '3',
                          '--warmup', '1', '--dump-outputs', str(tmp_path / 'dump')],
                         capture_output=True, text=True, timeout=600, cwd=str(REPO), env=dict(os.environ))
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line['metric'] == 'utterances_per_sec' and line['unit'] == 'utterances/s' and line['higher_is_better'] is True
    assert line['dtype'] == 'f32' and line['steps'] == 3 and line['full'] is False
    assert line['ms_per_step'] > 0 and line['value'] == pytest.approx(8 * 1e3 / line['ms_per_step'], rel=1e-9)
    assert line['p50_forward_ms'] is None and line['strong_proxy'] is None and 'cpu_baseline' not in line and 'roofline' not in line
    logits = np.load(tmp_path / 'dump' / 'logits.npy')
    assert logits.dtype == np.float32 and logits.shape == (8, 50, 49) and np.isfinite(logits).all()
