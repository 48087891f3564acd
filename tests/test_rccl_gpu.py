"""The RCCL path itself, on the one GPU of the test box (VERDICT r5 missing 1 / next 3).

`tests/test_distributed_cpu.py` covers the sharding arithmetic with gloo; what never ran before round 6 is
`parallel.py`'s `backend='nccl'` branch: `init_process_group('nccl', device_id=...)`, `all_gather_into_tensor`
/ `all_reduce` on DEVICE tensors, and their stream ordering against a pipelined forward's side stream.  RCCL
refuses two ranks on one device, so this is a ONE-rank nccl group with `force_collective=True`: the same
calls N ranks make (reference pattern replaced: training/torch/trainer.py:91-92, nn.DataParallel's gather).
Runs in a spawned process: a process group is process-global state.
"""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _rccl_worker(port, out_queue):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    import torch.distributed as dist
    import nb_asr_amd as nb
    from nb_asr_amd.parallel import ShardedForward
    from nb_asr_amd.weights import keyed_fill_, keyed_input
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    res = {}
    runner = ShardedForward(world_size=1, rank=0, device=dev, backend='nccl', force_collective=True)
    try:
        res['backend'] = dist.get_backend()
        res['collective'] = runner.collective
        model = nb.get_model([[3, 1], [4, 1, 1], [2, 1, 1, 1]], use_rnn=True, dropout_rate=0.0)
        keyed_fill_(model, 1235, 'lively')
        model = model.to(dev).eval()
        x = keyed_input(5, 61, seed=3).to(dev)
        with torch.no_grad():
            want = model(x).clone()
            res['forward'] = torch.equal(runner.forward(model, x), want)                 # forward + all_gather_into_tensor on the device
            res['forward_global'] = torch.equal(runner.forward_global(model, x), want)   # shard_bounds + the ragged gather
            res['gather_ragged'] = torch.equal(runner.gather_ragged(want, 5), want)
            # a pipelined forward writes its logits on the plan's side stream: the collective must be ordered behind it
            for _ in range(3):
                model.forward_async(x).result()
            handles = [model.forward_async(x) for _ in range(4)]
            gathered = [runner.gather_logits(h.result()) for h in handles]
            torch.cuda.synchronize()
            res['after_forward_async'] = all(torch.equal(g, want) for g in gathered)
            res['device'] = gathered[0].device.type
        # gradients: bucketed all-reduce on device tensors (several buckets), weighted by the shard size
        params = [torch.nn.Parameter(torch.full((1000,), float(i + 1), device=dev)) for i in range(5)]
        for p in params:
            p.grad = torch.full_like(p, 2.0)
        unused = torch.nn.Parameter(torch.ones(7, device=dev))
        runner.allreduce_gradients(params + [unused], bucket_bytes=8192, n_local=5)
        res['allreduce'] = all(bool((p.grad == 2.0).all()) for p in params) and bool((unused.grad == 0).all())
        res['max_over_ranks'] = runner.max_over_ranks(2.5)
        runner.barrier()
    finally:
        runner.close()
    out_queue.put(res)


@pytest.mark.gpu
def test_one_rank_rccl_group_runs_every_collective_of_the_path():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(_free_port(), q))
    p.start()
    res = q.get(timeout=600)
    p.join(timeout=120)
    assert p.exitcode == 0
    assert res['backend'] == 'nccl' and res['collective'] and res['device'] == 'cuda'
    assert res['forward'], 'forward + all-gather over RCCL differs from the plain forward'
    assert res['forward_global'] and res['gather_ragged']
    assert res['after_forward_async'], 'all-gather behind forward_async: logits differ (side-stream ordering)'
    assert res['allreduce'] and res['max_over_ranks'] == 2.5


@pytest.mark.gpu
def test_bench_force_collective_reports_the_allgather(tmp_path):
    """bench.py --force-collective: the N=1 line then includes the RCCL all-gather in every step and reports `allgather_us`."""
    import json
    import pathlib
    import subprocess
    import sys
    repo = pathlib.Path(__file__).resolve().parent.parent
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY='0')
    out = subprocess.run([sys.executable, str(repo / 'bench.py'), '--batch', '8', '--frames', '200', '--steps', '3', '--warmup', '1',
                          '--full', '--force-collective', '--no-cpu-baseline', '--no-strict', '--no-roofline'],
                         capture_output=True, text=True, timeout=900, env=env, cwd=str(repo))
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line['allgather_us'] is not None and line['allgather_us'] > 0
    assert 'RCCL' in line['config']['parallelism']
    assert line['strong_proxy'] is not None and line['strong_proxy']['per_gpu_batch'] == 1
