"""The per-frame GEMM (gemm_pointwise.hip), pinned to the bit: SHA-256 of every output tensor (whole, pitch columns included) and of
every packed weight tensor (every byte of it is written by the pack kernels), for both operand schemes, compared with a recording
made from the two-file kernels this one replaced (tests/golden/pointwise_bits.json).  No tolerance: the kernels are deterministic
(no atomics, one fixed K order), so a digest can only move if a sum was reordered or a rounding moved.  The activation workspace is
not digested: it has an unwritten gap between the inverse scales and the partial maxima.

The cases are the smallest shapes that reach each branch of the kernel (tile = 128 rows x 256 frames, K-step = 32 channels):

    L1  two frame tiles with ONE live frame in the second; K tail (n_ks = 2); three skips, a pending LayerNorm on x and on skip0
        (skip0 = x); frames t/2.. scaled by 1e-3, so the two tiles' scales differ
    L2  second row tile with two live rows (one active wave of eight); K tail of 4 channels; no skips
    L3  n_ks = 1: no prefetch, one barrier; one skip, no LayerNorm
    L4  n_ks = 3: the double buffer wraps; two skips; utterance 1 all zeros: tile maximum 0, the k = 0 branch of the pow2 scale
    P1  c_out = 272: n_mt = 3 > 2 n_nt b, the m-major tile order of the fp16 scheme; with LayerNorm
    P2  time-major store across two frame tiles and three utterances; no LayerNorm
    P3  the `_into` projection (fp16 scheme only): batch_total 5, batch_offset 2, with LayerNorm; the gate tensor is pre-filled with
        7.0 and digested whole, so untouched rows must stay 7.0

    python tests/test_pointwise_bits_gpu.py --record        # rewrites the fixture from the code as it is
"""
import hashlib
import json
import pathlib
import sys

import pytest
import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

import cases                                            # noqa: E402
from nb_asr_amd import hip                              # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIXTURE = REPO / 'tests' / 'golden' / 'pointwise_bits.json'
F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-3

# name: (entry, batch, c_in, c_out or hidden, frames, skips, LayerNorm, schemes)
SHAPES = {
    'L1': ('linear', 2, 40, 40, 257, 3, True, ('f16', 'bf16')),
    'L2': ('linear', 1, 36, 130, 5, 0, False, ('f16', 'bf16')),
    'L3': ('linear', 2, 24, 24, 37, 1, False, ('f16', 'bf16')),
    'L4': ('linear', 2, 72, 72, 300, 2, False, ('f16', 'bf16')),
    'P1': ('projection', 1, 40, 68, 5, 0, True, ('f16', 'bf16')),
    'P2': ('projection', 3, 72, 12, 259, 0, False, ('f16', 'bf16')),
    'P3': ('into', 2, 40, 12, 9, 0, True, ('f16',)),
}
CASES = [f'{name}-{scheme}' for name, spec in SHAPES.items() for scheme in spec[-1]]
INTO_TOTAL, INTO_OFFSET = 5, 2


def digest(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def rows(tag, b, c, t, dtype, scale=1.0):
    """(b, c, ld) activation of the storage type, pitch columns zero; the values are bf16-representable for the bf16 scheme."""
    out = torch.zeros(b, c, hip.row_pitch(t, dtype), dtype=dtype)
    out[:, :, :t] = cases.keyed_x(tag, (b, c, t), scale).to(dtype)
    return out


def run(case):
    """{'y': digest of the output tensor, 'packed': digest of the packed weights} of one case."""
    name, scheme = case.split('-')
    entry, b, c_in, c_out, t, n_skips, with_ln, _ = SHAPES[name]
    dtype = BF16 if scheme == 'bf16' else F32
    tag = f'pointwise_bits/{name}'
    rows_out = c_out if entry == 'linear' else 4 * c_out
    p = cases.keyed_params({'weight': (rows_out, c_in), 'bias': (rows_out,), 'bias_hh': (rows_out,), 'norm.weight': (c_in,), 'norm.bias': (c_in,)}, tag)
    p = {k: v.to(dtype).float().to(DEV) for k, v in p.items()}          # the fp32 VALUES of bf16 parameters for the bf16 scheme
    x = rows(tag, b, c_in, t, dtype)
    if name == 'L1':
        x[:, :, t // 2:] *= 1e-3
    if name == 'L4':
        x[1] = 0
    x = x.to(DEV)
    ld = x.shape[2]
    ln = None
    if with_ln:
        stats = torch.zeros(b, 2, ld, device=DEV)
        ln = (hip.channel_stats(x, stats, t, EPS), p['norm.weight'], p['norm.bias'])
    if scheme == 'bf16':
        packed, ws = hip.pack_pointwise_weights_bf16(p['weight']), hip.pointwise_bf16_workspace(b, c_in, ld, DEV)
    else:
        packed, ws = hip.pack_pointwise_weights(p['weight']), hip.pointwise_workspace(b, c_in, ld, DEV)
    if entry == 'linear':
        skips = [x if (name == 'L1' and i == 0) else rows(f'{tag}/skip{i}', b, c_out, t, dtype).to(DEV) for i in range(n_skips)]
        y = torch.full((b, c_out, ld), 7.0, dtype=dtype, device=DEV)
        fn = hip.linear_fused_bf16 if scheme == 'bf16' else hip.linear_fused_packed
        fn(x, t, packed, c_out, p['bias'], skips, y, ws, ln=ln, ln_on_x=with_ln, ln_on_skip0=with_ln and n_skips > 0)
    elif entry == 'projection':
        y = torch.full((t, b, rows_out), 7.0, device=DEV)
        fn = hip.lstm_input_projection_bf16 if scheme == 'bf16' else hip.lstm_input_projection_packed
        fn(x, t, packed, p['bias'], p['bias_hh'], y, c_out, ws, ln=ln)
    else:
        y = torch.full((t, INTO_TOTAL, rows_out), 7.0, device=DEV)
        hip.lstm_input_projection_packed(x, t, packed, p['bias'], p['bias_hh'], y, c_out, ws, ln=ln, batch_total=INTO_TOTAL, batch_offset=INTO_OFFSET)
    return {'y': digest(y), 'packed': digest(packed)}


@pytest.fixture(scope='module')
def pinned():
    return json.loads(FIXTURE.read_text())


def test_fixture_lists_exactly_the_cases(pinned):
    assert sorted(pinned) == sorted(CASES)


@pytest.mark.parametrize('case', CASES)
def test_pointwise_bits_are_the_recorded_ones(pinned, case):
    got = run(case)
    print(f'{case}: {got}')
    assert got == pinned[case]


if __name__ == '__main__':
    if sys.argv[1:] != ['--record']:
        raise SystemExit(__doc__)
    FIXTURE.write_text('{\n' + ',\n'.join(f'{json.dumps(case)}: {json.dumps(run(case))}' for case in CASES) + '\n}\n')
    print(f'wrote {len(CASES)} cases to {FIXTURE}')
