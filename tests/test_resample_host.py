"""The resampler without a GPU: the definition (resample_model.py) against the package's integer geometry and coefficient table, the stream's
host rules driven through the float64 model, the derived capacities, the C ABI's declarations and refusals."""
import ctypes
import math

import numpy as np
import pytest

from nb_asr_amd import frontend, hip, streaming
from nbasr_header import declarations
import resample_model as rm

PAIRS = [(r, 16000) for r in rm.RATES] + [(16000, r) for r in rm.RATES]
# what the issue's float64 check of the definition found, as expectations of the derivation: (taps, retained samples, pending outputs)
EXPECTED = {8000: (13, 12, 12), 11025: (13, 11, 9), 22050: (17, 16, 6), 32000: (25, 24, 6), 44100: (34, 32, 6), 48000: (37, 36, 6)}


@pytest.mark.parametrize('orig', rm.RATES)
def test_integer_support_is_the_open_interval_of_six_periods(orig):
    """|m n - j o| min(o, n) 99 < 600 o n exactly where |t| < 6, for every phase and every sample near the support's edges (t is a
    ratio of integers: the comparison is made in integers scaled by 100 o n, without rounding)."""
    o, n = rm.ratio(orig, 16000)
    assert (o, n) == frontend.resample_ratio(orig, 16000)
    for j in list(range(n)) + [n + 3, 5 * n + 1]:
        lo, hi = frontend.resample_support(j, o, n)
        assert (lo, hi) == rm.support(j, o, n)
        for m in range(lo - 3, hi + 4):
            inside = lo <= m <= hi
            assert inside == rm.inside(m, j, o, n)
            assert inside == (abs(rm.time_of(m, j, o, n)) < 6.0 - 1e-9) or abs(abs(rm.time_of(m, j, o, n)) - 6.0) < 1e-9
            assert inside == (abs(m * n - j * o) * 99 * min(o, n) < 600 * o * n)
    assert frontend.resample_taps(o, n) == rm.largest_support(o, n)


@pytest.mark.parametrize('orig,new', PAIRS)
def test_table_form_equals_absolute_form(orig, new):
    o, n = rm.ratio(orig, new)
    table = frontend.resample_table(o, n)
    taps = frontend.resample_taps(o, n)
    assert table.shape == (n, taps | 1) and taps <= frontend.RESAMPLE_MAX_TAPS and max(o, n) <= frontend.RESAMPLE_MAX_RATIO
    for j in sorted({0, 1, n - 1, n, 2 * n + n // 2, 7 * n + n // 3}):
        p, k = j % n, j // n
        lo, hi = frontend.resample_support(p, o, n)
        assert (lo + k * o, hi + k * o) == rm.support(j, o, n)
        want = [rm.coefficient(m, j, o, n) for m in range(lo + k * o, hi + k * o + 1)]
        # the absolute form subtracts m / o and j / n, each up to ~8 periods here and rounded to 2^-53 relative: 8 * 2^-52 in the
        # difference, times base <= 437, in t; |dh/dt| < 2: below 2e-12
        np.testing.assert_allclose(table[p, :hi - lo + 1], want, rtol=0, atol=2e-12)
        assert not table[p, hi - lo + 1:].any()


@pytest.mark.parametrize('orig', rm.RATES)
def test_dc_gain_and_tone(orig):
    """Loose, stated bounds on what the filter does: DC gain within 2e-3 of 1, a 1 kHz tone reproduced to 2e-3 (away from the ends)."""
    o, n = rm.ratio(orig, 16000)
    L = 40 * max(o, 8) if o < 100 else 3 * o
    y, _ = rm.resample64(np.ones(L), o, n)
    mid = slice(40, len(y) - 40)
    assert np.max(np.abs(y[mid] - 1.0)) < 2e-3
    tone, _ = rm.resample64(np.sin(2 * math.pi * 1000.0 * np.arange(L) / orig), o, n)
    want = np.sin(2 * math.pi * 1000.0 * np.arange(len(tone)) / 16000.0)
    assert np.max(np.abs(tone[mid] - want[mid])) < 2e-3


@pytest.mark.parametrize('orig', (8000, 44100, 48000))
def test_float32_form_meets_the_derived_bound(orig):
    """The kernel's order of evaluation, on the host: within (taps + 2) 2^-24 sum |h x| of the float64 form."""
    o, n = rm.ratio(orig, 16000)
    x = np.random.default_rng(orig + 1).standard_normal(2 * o + 300).astype(np.float32)
    y, bound = rm.resample64(x, o, n)
    assert np.all(np.abs(rm.resample32(x, o, n) - y) <= rm.error_bound(bound, rm.largest_support(o, n)))


def test_an_11_khz_tone_at_48_khz_is_suppressed():
    o, n = rm.ratio(48000, 16000)
    y, _ = rm.resample64(np.sin(2 * math.pi * 11000.0 * np.arange(1500) / 48000.0), o, n)
    assert np.max(np.abs(y[40:-40])) < 1e-2


@pytest.mark.parametrize('orig,new', PAIRS)
def test_final_count_is_monotone_and_below_every_total(orig, new):
    o, n = rm.ratio(orig, new)
    prev = 0
    for s in range(0, 3 * o + 80):
        f = frontend.resample_final(s, o, n)
        assert f >= prev and f == rm.final(s, o, n)
        assert all(f <= frontend.resample_total(L, o, n) for L in range(s, s + 3))       # (total is monotone in L)
        assert frontend.resample_total(s, o, n) == rm.total(s, o, n) == math.ceil(n * s / o)
        assert frontend.resample_peek(s, o, n) == frontend.resample_total(s, o, n) - f >= 0
        prev = f


@pytest.mark.parametrize('orig', rm.RATES)
def test_float64_model_through_the_host_geometry_is_the_whole_utterance(orig):
    """Pushes of 1, 0, 7, o, o + 1, 3 o, 50, ... samples: the outputs the host rules release, computed from the retained tail and the
    push alone, are exactly the whole utterance's, and no output reads a sample the tail no longer holds."""
    o, n = rm.ratio(orig, 16000)
    rng = np.random.default_rng(orig)
    L = 4 * o + 700
    x = rng.standard_normal(L)
    whole, _ = rm.resample64(x, o, n)
    cap = frontend.resample_tail_capacity(o, n)
    sizes = [1, 0, 7, o, o + 1, 3 * o, 50, 2, 441, 5]
    s = out = first = i = 0
    got, most_tail, most_pending = [], 0, 0
    tail = np.zeros(0)

    def output(j, held, held_first, length):
        taps = rm.taps_of(j, length, o, n)
        assert taps[0][0] >= held_first and taps[-1][0] < held_first + len(held), (j, taps[0][0], taps[-1][0], held_first, len(held))
        acc = 0.0
        for m, h in taps:
            acc += h * float(held[m - held_first])
        return acc

    while s < L:
        push = x[s:min(L, s + sizes[i % len(sizes)])]
        i += 1
        held = np.concatenate([tail, push])
        s += len(push)
        f = frontend.resample_final(s, o, n)
        got += [output(j, held, first, s) for j in range(out, f)]
        out = f
        new_first = frontend.resample_retain_from(out, o, n)
        tail, first = held[new_first - first:], new_first
        assert len(tail) <= cap
        most_tail, most_pending = max(most_tail, len(tail)), max(most_pending, frontend.resample_total(s, o, n) - out)
    got += [output(j, tail, first, L) for j in range(out, frontend.resample_total(L, o, n))]
    assert np.array_equal(np.array(got), whole)
    assert most_tail <= cap and most_pending <= frontend.resample_max_pending(o, n)


@pytest.mark.parametrize('orig', rm.RATES)
def test_capacities_are_the_derived_ones(orig):
    o, n = rm.ratio(orig, 16000)
    taps, retained, pending = EXPECTED[orig]
    assert frontend.resample_taps(o, n) == taps
    # brute force over three periods past the start-up, with the model's own counts
    states = range(0, 4 * o + 100)
    cap = max(s - max(0, rm.support(rm.final(s, o, n), o, n)[0]) for s in states)
    most = max(rm.total(s, o, n) - rm.final(s, o, n) for s in states)
    # (EXPECTED was seen with one push pattern; over every cut the retained samples and pending outputs reach one more at some rates)
    assert frontend.resample_tail_capacity(o, n) == cap == 2 * frontend.resample_reach(o, n) // n and retained <= cap <= retained + 1
    assert frontend.resample_max_pending(o, n) == most and pending <= most <= pending + 1
    assert frontend.resample_lookahead(o, n) == max(rm.support(j, o, n)[1] - (j * o) // n for j in range(n))
    r = frontend.Resampler(orig, device='cuda:0')                   # (no device is touched before the first use)
    assert (r.o, r.n, r.taps, r.tail_capacity, r.max_pending) == (o, n, taps, cap, most)
    assert r.out_len(1000) == rm.total(1000, o, n)


def test_end_frame_bound():
    """frames_total(s + pending) - frames_final(s) at its largest; 2 without a resampler, 2 for the six rates, 3 from 194 pending on."""
    for pending in (0, 6, 12, 120, 121, 200):
        want = max(frontend.frames_total(s + pending) - frontend.frames_final(s) for s in range(201, 1200))
        assert frontend.end_frames_bound(pending) == want
    assert frontend.end_frames_bound(0) == 2 and frontend.end_frames_bound(121) == 3
    for orig in rm.RATES:
        assert frontend.end_frames_bound(frontend.Resampler(orig).max_pending) == 2
    planner = streaming.StreamPlanner(streaming.stage_specs([['conv5', 0], ['conv5', 0, 0], ['conv5', 0, 0, 0]]))
    assert planner.max_provisional_frames() == planner.max_provisional_frames(2) <= planner.max_provisional_frames(3)


def test_abi_declarations():
    decl = declarations()
    for name in ('nbasr_resample_state_bytes', 'nbasr_resample_stream_step', 'nbasr_resample'):
        assert name in decl and name in hip.SIGNATURES
        assert len(hip.SIGNATURES[name][1]) == len(decl[name][1])
    assert hip.ABI_VERSION == 6
    assert 'const int* lengths' in decl['nbasr_resample'][1]
    lib = hip.load_library()
    assert lib.nbasr_resample_state_bytes(3, 36) == 2 * 3 * 36 * 4 and lib.nbasr_resample_state_bytes(3, 33) == 2 * 3 * 36 * 4
    assert lib.nbasr_resample_state_bytes(0, 36) == 0 and lib.nbasr_resample_state_bytes(3, 0) == 0


def step(lib, tail_in=32, tail_len=0, tail_first=0, wave=64, n_new=100, ld_wave=None, tail_out=None, rel=0, cap=36, table=128, orig=48000,
         new=16000, out=256, ld_out=64, col0=0, first_out=0, n_out=0, final=0, batch=1):
    """nbasr_resample_stream_step with made-up (never dereferenced) addresses: every call here is refused on the host."""
    total = tail_first + tail_len + n_new
    return lib.nbasr_resample_stream_step(tail_in, tail_len, tail_first, wave, n_new, n_new if ld_wave is None else ld_wave, tail_out, rel, cap,
                                          table, orig, new, out, ld_out, col0, first_out, n_out, total, final, batch, None)


def test_entry_points_refuse_bad_arguments_on_the_host():
    lib = hip.load_library()
    err = lib.nbasr_last_error
    assert step(lib, orig=0, n_out=1) == -1 and b'positive' in err()
    assert step(lib, new=-16000, n_out=1) == -1 and b'positive' in err()
    assert step(lib, orig=16000, new=16001, n_out=1) == -1 and b'limits' in err()          # coprime: 16000 : 16001
    assert step(lib, orig=1000, new=48, n_out=1) == -1 and b'taps' in err()                # 125 : 6, a support of 253 samples
    assert step(lib, n_out=29, first_out=0) == -1 and b'need samples' in err()             # output 28 needs samples up to 102 of 100
    assert step(lib, n_out=27, first_out=0, ld_out=16) == -1 and b'do not fit' in err()
    assert step(lib, tail_first=1000, tail_len=30, n_new=60, first_out=330, n_out=2) == -1 and b'need samples' in err()   # sample 972 is gone
    assert step(lib, n_out=40, final=1) == -1 and b'beyond' in err()                       # 100 samples make 34 outputs
    assert step(lib, tail_out=36) == -2 and b'16-byte' in err()
    assert step(lib, tail_in=32, tail_out=32) == -1 and b'in turn' in err()
    assert step(lib, rel=0, tail_out=48) == -1 and b'retaining 100 samples' in err()
    assert step(lib, rel=101, tail_out=48) == -1
    assert step(lib, cap=0) == -1 and b'tail_capacity' in err()
    assert step(lib, tail_len=37) == -1 and step(lib, batch=70000, n_out=1) == -1
    # whole utterances
    assert lib.nbasr_resample(64, 100, 100, None, 128, 48000, 16000, 256, 34, 33, 1, None) == -1 and b'make 34 outputs' in err()
    assert lib.nbasr_resample(64, 100, 100, None, 128, 0, 16000, 256, 34, 34, 1, None) == -1 and b'positive' in err()
    assert lib.nbasr_resample(64, 99, 100, None, 128, 48000, 16000, 256, 34, 34, 1, None) == -1
    assert lib.nbasr_resample(64, 100, 100, None, None, 48000, 16000, 256, 34, 34, 1, None) == -3
    assert lib.nbasr_resample(64, 100, 100, None, 128, 48000, 16000, 256, 34, 34, 0, None) == 0     # nothing to do


def test_python_refusals_need_no_device():
    for bad in ((0, 16000), (-8000, 16000), (8000, 0)):
        with pytest.raises(ValueError, match='positive'):
            frontend.Resampler(*bad)
    with pytest.raises(ValueError, match='limit'):
        frontend.Resampler(16001, 16000)
    with pytest.raises(ValueError, match='taps'):
        frontend.Resampler(1000, 48)
    for r in rm.RATES:                                       # the six rates pass, in both directions
        frontend.Resampler(r, 16000), frontend.Resampler(16000, r)
    with pytest.raises(ValueError, match='batch must be positive'):
        frontend.ResamplerStream(frontend.Resampler(48000), 0)
    # the session: no rate without a front-end; the front-end's own rate is no resampler; max_chunk below the end frames is refused
    cls = streaming.StreamingSession
    with pytest.raises(ValueError, match='front-end'):
        cls.resampler_for(None, 48000, None)
    fe = object.__new__(frontend.LogMelFrontend)
    fe.sample_rate, fe.hop_length, fe.n_fft = 16000, 160, 400
    assert cls.resampler_for(fe, None, 'cuda:0') is None and cls.resampler_for(fe, 16000, 'cuda:0') is None
    r = cls.resampler_for(fe, 48000, 'cuda:0')
    assert isinstance(r, frontend.Resampler) and (r.o, r.n) == (3, 1)
    assert cls.check_max_chunk(1, None, None) == 2 and cls.check_max_chunk(1, fe, None) == 2      # as before: any max_chunk >= 1
    assert cls.check_max_chunk(2, fe, r) == 2
    with pytest.raises(ValueError, match='max_chunk=1 is below the 2 frames'):
        cls.check_max_chunk(1, fe, r)
    for name in ('push', 'flush', 'peek', 'reset'):
        assert callable(getattr(frontend.ResamplerStream, name))
    assert callable(hip.resample) and callable(hip.resample_stream_step) and callable(hip.resample_state_bytes)
