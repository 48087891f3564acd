#!/usr/bin/env python3
"""Known answers of the reference package for the drop-in boundary tests (tests/test_reference_registration.py,
tests/test_bench_dataset.py::test_reference_loader_reads_the_file), so that those tests run without a reference checkout.

Records only data:
  registration   what the reference's own get_model(..., backend='hip') returned once nb_asr_amd.register_with() had seeded its
                 backend accessor (type, parameter count, training mode; with and without default=True), and the state_dict keys
                 and shapes of the reference's torch backend model for the same architecture (checkpoints move unchanged)
  bench_dataset  the header and rows of the benchmarking files nb_asr_amd.bench_dataset wrote (one device; two devices), as the
                 reference's BenchmarkingDataset read them, and that loader's answers to the queries the test makes

Run where a checkout of the reference is available:  python tests/golden/make_reference_answers.py PATH_TO_REFERENCE_CHECKOUT"""
import json
import pathlib
import pickle
import sys
import tempfile

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(pathlib.Path(sys.argv[1]).resolve()))
sys.dont_write_bytecode = True

import nasbench_asr as ref  # noqa: E402
from nasbench_asr import dataset as ref_dataset  # noqa: E402

import nb_asr_amd  # noqa: E402
from nb_asr_amd import bench_dataset, search_space  # noqa: E402

ARCH_REG = [[3, 1], [4, 1, 1], [2, 1, 1, 1]]
ARCH_DS = [[1, 0], [1, 0, 0], [1, 0, 0, 0]]


def shapes(model):
    return {k: list(v.shape) for k, v in model.state_dict().items()}


def registration():
    backends = ref.model._backends
    saved = dict(backends.backends), list(backends.available_backends)
    try:
        theirs = ref.get_model(ARCH_REG, use_rnn=True, dropout_rate=0.0, backend='torch')
        out = {'arch': ARCH_REG, 'torch_backend_state_dict_shapes': shapes(theirs),
               'torch_backend_type_module': type(theirs).__module__}
        assert nb_asr_amd.register_with(ref) == 'hip'
        model = ref.get_model(ARCH_REG, use_rnn=True, dropout_rate=0.0, backend='hip')
        out['hip'] = {'type': f'{type(model).__module__}.{type(model).__qualname__}', 'training': model.training,
                      'parameters': sum(p.numel() for p in model.parameters()), 'backend_attr': model.backend,
                      'hip_available': 'hip' in ref.model.get_available_backends()}
        nb_asr_amd.register_with(ref, default=True)
        model = ref.get_model(ARCH_REG, use_rnn=False, dropout_rate=0.0)
        out['default_no_rnn'] = {'type': f'{type(model).__module__}.{type(model).__qualname__}',
                                 'parameters': sum(p.numel() for p in model.parameters()), 'use_rnn': model.use_rnn}
        return out
    finally:
        backends.backends.clear()
        backends.backends.update(saved[0])
        backends.available_backends[:] = saved[1]


def rows():
    return [[search_space.get_model_hash(a), 0.01 * (i + 1)] for i, a in enumerate((ARCH_DS, [[3, 1], [4, 1, 1], [2, 1, 1, 1]],
                                                                                   [[0, 1], [5, 1, 0], [2, 0, 1, 1]]))]


def read_back(path):
    with open(path, 'rb') as f:
        return {'header': pickle.load(f), 'rows': pickle.load(f)}


def bench_dataset_answers():
    with tempfile.TemporaryDirectory() as d:
        path, path8 = pathlib.Path(d) / bench_dataset.file_name('mi355x-fp32'), pathlib.Path(d) / bench_dataset.file_name('mi355x-fp32-x8')
        bench_dataset.write_benchmarking_dataset(path, 'mi355x-fp32', rows())
        ds = ref_dataset.BenchmarkingDataset([str(path)])
        one = {'file': read_back(path), 'devices': ds.devices, 'columns': ds.columns[:2], 'latency_arch': ds.latency(ARCH_DS),
               'latency_arch_dict': ds.latency(ARCH_DS, return_dict=True), 'latency_absent': ds.latency([[5, 0], [5, 0, 0], [5, 0, 0, 0]]),
               'arch_in': ARCH_DS in ds}
        bench_dataset.write_benchmarking_dataset(path8, 'mi355x-fp32-x8', [[h, 2 * v] for h, v in rows()], meta={'n_gpus': 8})
        bench_dataset.write_benchmarking_dataset(path, 'mi355x-fp32', rows(), meta={'n_gpus': 1})
        both = ref_dataset.BenchmarkingDataset([str(path), str(path8)])
        two = {'file_x8': read_back(path8), 'devices': both.devices, 'latency_arch_dict': both.latency(ARCH_DS, return_dict=True)}
    return {'arch': ARCH_DS, 'rows': rows(), 'one_device': one, 'two_devices': two}


answers = {'registration': registration(), 'bench_dataset': bench_dataset_answers()}
out = HERE / 'reference_answers.json'
out.write_text(json.dumps(answers, indent=1, sort_keys=True) + '\n')
print(f'wrote {out}')
