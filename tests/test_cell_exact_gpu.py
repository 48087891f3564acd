"""The grouped-convolution cells and node kernels against an fp64 evaluation, to the bit, on exactly summable operands.

``tests/cell_exact.py`` builds operands on which every product and every partial sum of a cell is a small integer (exact in bfloat16 and
float32 whatever the order of the sums) and evaluates the reference's cell in fp64; ``tests/test_cell_exact_host.py`` shows without a GPU
that the comparison is not blind.  Here every kernel of the family must give the reference's x3 as numbers, element by element:

* ``nbasr_grouped_cell_mfma`` at every tiling ``NBASR_CELLM_TILING`` can force, at the frame counts that reach the edges of its 8-frame
  global chunk, its 16-frame column block, the partner column block of the 8-slot form, and the row end at, before and after a wave-tile
  seam; on a pitch that leaves a wave tile wholly past the row end; with 5 and 6 groups on the planner's own tiling; every utterance of a
  batch also alone, bit for bit;
* ``nbasr_grouped_cell_fused`` with either storage type (and its output-channel split forced off and on) and three
  ``nbasr_grouped_conv1d_node`` launches at every ``NBASR_GC_*`` variant, around the 4-frame lane chunk and the 256-frame wave, with the
  statistics by-product against fp64 statistics of the reference's x3;
* one weight moved to the neighbouring tap in the kernels' copy only is noticed by both cells.

Every launch writes into the middle of a NaN-filled allocation: the guards stay NaN, the pitch columns are zero.
"""
import pytest
import torch

import cases
import cell_exact as ce
from nb_asr_amd import hip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF = torch.bfloat16
NAN = float('nan')
GUARD = 64                      # elements on either side of y: 128 / 256 bytes, y stays 16-byte aligned
STATS_EPS = 1e-3
STATS_RTOL, STATS_ATOL = 1e-5, 2e-6          # test_grouped_conv_epilogue_statistics (tests/test_ops_gpu.py)


# ---- launches into guarded allocations -------------------------------------------------------------------------------------------------
def guarded(b, c, ld, dtype):
    """(the whole NaN-filled allocation, y (b, c, ld) as a view of its middle)."""
    n = b * c * ld
    whole = torch.full((n + 2 * GUARD,), NAN, dtype=dtype, device=DEV)
    y = whole[GUARD:GUARD + n].view(b, c, ld)
    assert y.data_ptr() % 16 == 0
    return whole, y


def assert_written(whole, y, t, what):
    assert bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[-GUARD:]).all()), f'{what}: wrote outside y'
    assert bool((y[:, :, t:] == 0).all()), f'{what}: pitch columns are not zero'


def assert_exact(y, t, want, what):
    """torch.equal on values (-0.0 equals 0.0) over all frames < t."""
    got = y[:, :, :t].double().cpu()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        u, ch, f = bad[0].tolist()
        raise AssertionError(f'{what}: {len(bad)} of {want.numel()} elements differ from fp64; first at (utterance, channel, frame) = '
                             f'{(u, ch, f)}: got {float(got[u, ch, f])}, want {float(want[u, ch, f])}; frames {sorted(set(bad[:, 2].tolist()))[:24]}')


def device_operands(case, dtype, ld, ops=None):
    """x0 (zero pitch columns), the pending LayerNorm as (stats (b, 2, ld), gamma, beta) or None, and the nodes with fp32 weights."""
    ops = ce.operands(case) if ops is None else ops
    b, c, t = ops.x0.shape
    x = torch.zeros(b, c, ld, dtype=dtype, device=DEV)
    x[:, :, :t] = ops.x0.to(dtype).to(DEV)
    ln = None
    if ops.ln is not None:
        mean, rstd, gamma, beta = ops.ln
        stats = torch.zeros(b, 2, ld, device=DEV)
        stats[:, 0, :t], stats[:, 1, :t] = mean.float().to(DEV), rstd.float().to(DEV)
        ln = (stats, gamma.float().to(DEV), beta.float().to(DEV))
    nodes = [(w.float().to(DEV).contiguous(), bias.float().to(DEV), k, d) for w, bias, k, d in ops.nodes]
    return x, ln, nodes


def bits(y):
    return y.contiguous().view(torch.int16 if y.dtype == BF else torch.int32)


# ---- the matrix-core cell ----------------------------------------------------------------------------------------------------------------
def mfma_launch(case, x, ln, packed, rows=slice(None)):
    xs = x[rows]
    whole, y = guarded(xs.shape[0], xs.shape[1], xs.shape[2], BF)
    hip.grouped_cell_mfma(xs, packed, case.mask, y, case.t, case.groups, None if ln is None else (ln[0][rows], ln[1], ln[2]))
    torch.cuda.synchronize()
    return whole, y


def mfma_check(case, ld, monkeypatch, tilings, want=None, ops=None):
    """The case at pitch ld on each of `tilings` ((nbt, gpw), or None for the planner's own): the batch equals the fp64 x3, every
    utterance alone equals its rows of the batch bit for bit.  Returns the tilings that ran (the entry point refuses those that do not
    fit the row)."""
    want = ce.reference(case).x3 if want is None else want
    x, ln, nodes = device_operands(case, BF, ld, ops)
    packed = [(hip.grouped_cell_mfma_pack(w, case.groups), bias, k, d) for w, bias, k, d in nodes]
    ran = []
    for tiling in tilings:
        if tiling is None:
            monkeypatch.delenv('NBASR_CELLM_TILING', raising=False)
        else:
            monkeypatch.setenv('NBASR_CELLM_TILING', f'{tiling[0]},{tiling[1]}')
        what = f'{case} ld {ld} tiling {tiling}'
        try:
            whole, y = mfma_launch(case, x, ln, packed)
        except hip.HipError as e:
            if tiling is not None and 'does not fit this row' in str(e):
                continue
            raise
        ran.append(tiling)
        assert_written(whole, y, case.t, what)
        assert_exact(y, case.t, want, what)
        for i in range(case.batch):
            whole_i, y_i = mfma_launch(case, x, ln, packed, slice(i, i + 1))
            assert_written(whole_i, y_i, case.t, f'{what} utterance {i} alone')
            assert torch.equal(bits(y_i), bits(y[i:i + 1])), f'{what}: utterance {i} alone differs from its rows of the batch'
    print(f'cg {case.cg} groups {case.groups} t {case.t} ld {ld} mask {case.mask}: ran {ran}, refused {[v for v in tilings if v not in ran]}')
    return ran


def expected_to_fit(cg, nbt, ld):
    """The forced tilings that fit a row of these cases (4 groups, <= 784 frames of pitch): all but one.  Four 16-slot groups of three
    256-frame wave tiles need 4 x 2 tiles x (4 planes x 800 frames x 8 bytes + 256) = 202 KiB of LDS, more than a CU's 160 KiB; with two
    tiles per row (138 KiB) or two groups per workgroup (101 KiB) they fit.  A tiling that is refused anywhere else is a finding."""
    return [(nbt, gpw) for gpw in ce.MFMA_GPWS if not (cg > 8 and nbt == 16 and gpw == 4 and ld > 512)]


@pytest.mark.parametrize('cg,nbt,t', ce.mfma_forced_cases())
def test_matrix_core_cell_equals_fp64_at_every_forced_tiling(cg, nbt, t, monkeypatch):
    """Every (blocks per wave, groups per workgroup) at the frame counts of ``cell_exact.mfma_frames``: 4 groups, 2 utterances, with the
    pending LayerNorm and skips 0b101001 and without it and skips 0b010110."""
    for combo in ce.COMBOS:
        ld = hip.row_pitch(t, BF)
        ran = mfma_check(ce.case(cg, t, combo), ld, monkeypatch, [(nbt, gpw) for gpw in ce.MFMA_GPWS])
        assert ran == expected_to_fit(cg, nbt, ld), (cg, nbt, t, ran)


@pytest.mark.parametrize('cg,nbt,t', ce.mfma_wide_pitch_cases())
def test_matrix_core_cell_with_a_wave_tile_wholly_past_the_row_end(cg, nbt, t, monkeypatch):
    """A pitch one wave tile larger than the row needs: the row ends one frame into its second tile, a third tile holds pitch columns
    only -- it loads, computes and stores zeros, and the taps of the tile before it read them."""
    ld = hip.row_pitch(t, BF) + 16 * nbt
    assert ld % 8 == 0 and -(-ld // (16 * nbt)) == 3
    for combo in ce.COMBOS:
        ran = mfma_check(ce.case(cg, t, combo), ld, monkeypatch, [(nbt, gpw) for gpw in ce.MFMA_GPWS])
        assert ran == expected_to_fit(cg, nbt, ld), (cg, nbt, t, ran)


@pytest.mark.parametrize('case', ce.mfma_other_cases(), ids=lambda c: f'cg{c.cg}-g{c.groups}-t{c.t}-m{c.mask}')
def test_matrix_core_cell_on_the_planners_tiling_with_every_skip_none_and_odd_group_counts(case, monkeypatch):
    """Every skip and no skip (4 groups), and 5 and 6 groups -- the last group of a launch whose group count is no multiple of 4 -- on the
    tiling the planner takes; for launches this small that is one group per workgroup, so the smallest tile is also forced with every
    groups-per-workgroup the group count allows (6 groups: 2, the last workgroup's second group being the launch's last)."""
    ld = hip.row_pitch(case.t, BF)
    assert hip.grouped_cell_mfma_fits(case.cg * case.groups, ld, case.groups) in (1, 2, 4)
    forced = [(8, gpw) for gpw in ce.MFMA_GPWS if case.groups % gpw == 0]
    ran = mfma_check(case, ld, monkeypatch, [None] + forced)
    assert ran == [None] + forced, ran
    if case.groups % 4:                                                  # a groups-per-workgroup that does not divide the groups is refused
        assert mfma_check(case, ld, monkeypatch, [(8, 4)]) == []


# ---- the vector cell and the node kernels ----------------------------------------------------------------------------------------------------
def node_variants(dtype):
    """Every NBASR_GC_* combination nbasr_grouped_conv1d_node takes for the storage type (walk.py and the variant table choose among them)."""
    base = (0, hip.GC_FPL8, hip.GC_WPERM, hip.GC_FPL8 | hip.GC_WPERM)
    return base + ((hip.GC_OSPLIT, hip.GC_PIPE, hip.GC_PIPE | hip.GC_OSPLIT, hip.GC_RING) if dtype == torch.float32 else ())


def assert_statistics(ws, case, ld, groups_per_part, what):
    """The partials a launch left in ws, merged, against fp64 statistics of the reference's x3."""
    b, c, t = case.batch, case.cg * case.groups, case.t
    got = torch.full((b, 2, ld), NAN, device=DEV)
    hip.grouped_stats_finalize(ws, got, c, t, case.groups, STATS_EPS, groups_per_part)
    mean, rstd = ce.statistics(ce.reference(case).x3, STATS_EPS)
    got = got.cpu()
    assert bool(torch.isfinite(got).all()) and bool((got[:, :, t:] == 0).all()), what
    r_mean = cases.worst_ratio(got[:, 0, :t], mean, STATS_RTOL, STATS_ATOL)
    r_rstd = cases.worst_ratio(got[:, 1, :t], rstd, STATS_RTOL, STATS_ATOL)
    print(f'{what}: statistics reach {r_mean:.3f} (mean) and {r_rstd:.3f} (rstd) of the tolerance')
    assert r_mean <= 1.0 and r_rstd <= 1.0, (what, r_mean, r_rstd)


def vector_cell(case, dtype, monkeypatch):
    b, c, t = case.batch, case.cg * case.groups, case.t
    ld = hip.row_pitch(t, dtype)
    x, ln, nodes = device_operands(case, dtype, ld)
    packed = [(hip.pack_grouped_weights(w, case.groups), bias, k, d) for w, bias, k, d in nodes]
    gpp = hip.grouped_cell_fits(c, ld, case.groups)
    assert gpp in (1, 2, 4)
    want = ce.reference(case).x3
    splits = (None, '0', '1') if dtype == torch.float32 and case.cg in (8, 12) else (None,)     # (the output-channel split has these instantiations)
    for split in splits:
        if split is None:
            monkeypatch.delenv('NBASR_CELL_OS', raising=False)
        else:
            monkeypatch.setenv('NBASR_CELL_OS', split)
        for with_stats in (False, True):
            what = f'{case} {dtype} cell, NBASR_CELL_OS={split}, statistics {with_stats}'
            ws = hip.grouped_stats_workspace(b, ld, case.groups, DEV) if with_stats else None
            whole, y = guarded(b, c, ld, dtype)
            hip.grouped_cell_fused(x, packed, case.mask, y, t, case.groups, ln, ws)
            torch.cuda.synchronize()
            assert_written(whole, y, t, what)
            assert_exact(y, t, want, what)
            if with_stats:
                assert_statistics(ws, case, ld, gpp, what)
    monkeypatch.delenv('NBASR_CELL_OS', raising=False)


def node_launches(case, dtype, variant):
    b, c, t, groups = case.batch, case.cg * case.groups, case.t, case.groups
    ld = hip.row_pitch(t, BF if (dtype == BF or variant & hip.GC_FPL8) else torch.float32)       # 16-byte lanes: 8 frames where a lane moves 8
    x, ln, nodes = device_operands(case, dtype, ld)
    if variant & hip.GC_WPERM:
        nodes = [(hip.pack_grouped_weights(w, groups), bias, k, d) for w, bias, k, d in nodes]
    ref = ce.reference(case)
    s = [bool(case.mask >> i & 1) for i in range(6)]
    with_stats = not variant & hip.GC_OSPLIT                              # (the output-split kernels have no statistics epilogue)
    ws = hip.grouped_stats_workspace(b, ld, groups, DEV) if with_stats else None
    (w1, x1), (w2, x2), (w3, x3) = (guarded(b, c, ld, dtype) for _ in range(3))
    hip.grouped_conv1d_node(x, *nodes[0][:2], [x] if s[0] else [], x1, t, groups, *nodes[0][2:], ln, ln is not None, ln is not None and s[0], None, variant)
    hip.grouped_conv1d_node(x1, *nodes[1][:2], ([x] if s[1] else []) + ([x1] if s[2] else []), x2, t, groups, *nodes[1][2:],
                            ln if s[1] else None, False, ln is not None and s[1], None, variant)
    hip.grouped_conv1d_node(x2, *nodes[2][:2], ([x] if s[3] else []) + ([x1] if s[4] else []) + ([x2] if s[5] else []), x3, t, groups,
                            *nodes[2][2:], ln if s[3] else None, False, ln is not None and s[3], ws, variant)
    torch.cuda.synchronize()
    for name, whole, y, want in (('x1', w1, x1, ref.x1), ('x2', w2, x2, ref.x2), ('x3', w3, x3, ref.x3)):
        what = f'{case} {dtype} node launches, variant {variant}, {name}'
        assert_written(whole, y, t, what)
        assert_exact(y, t, want, what)
    if with_stats:
        assert_statistics(ws, case, ld, 4, f'{case} {dtype} node launches, variant {variant}')


@pytest.mark.parametrize('dtype', [torch.float32, BF], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', ce.vector_cases(), ids=lambda c: f'cg{c.cg}-t{c.t}-m{c.mask}')
def test_vector_cell_and_node_kernels_equal_fp64(case, dtype, monkeypatch):
    """nbasr_grouped_cell_fused and three nbasr_grouped_conv1d_node launches per variant, either storage type, at 1, 3, 4, 5, 255, 256, 257
    and 513 frames: x3 (the node launches: x1 and x2 as well) equals the fp64 reference; the statistics by-product, merged, equals fp64
    statistics of the reference's x3 to the tolerance of test_grouped_conv_epilogue_statistics."""
    vector_cell(case, dtype, monkeypatch)
    for variant in node_variants(dtype):
        node_launches(case, dtype, variant)


# ---- sensitivity -------------------------------------------------------------------------------------------------------------------------
def test_one_weight_on_the_neighbouring_tap_is_noticed_by_both_cells(monkeypatch):
    """The kernels get a copy of the operands in which one nonzero weight of the last node sits on the neighbouring tap: their x3 is the
    fp64 evaluation of THAT copy, and no longer the reference's -- the equality above is not vacuous."""
    case = ce.SENSITIVITY
    moved, _ = ce.move_one_tap(ce.operands(case))
    want, want_moved = ce.reference(case).x3, ce.evaluate(moved, case).x3
    assert not torch.equal(want, want_moved)
    t, b, c = case.t, case.batch, case.cg * case.groups
    ld = hip.row_pitch(t, BF)
    assert mfma_check(case, ld, monkeypatch, [None], want_moved, moved) == [None]
    x, ln, nodes = device_operands(case, BF, ld, moved)
    packed = [(hip.grouped_cell_mfma_pack(w, case.groups), bias, k, d) for w, bias, k, d in nodes]
    _, y = mfma_launch(case, x, ln, packed)
    assert not torch.equal(y[:, :, :t].double().cpu(), want)
    for dtype in (torch.float32, BF):
        ld = hip.row_pitch(t, dtype)
        x, ln, nodes = device_operands(case, dtype, ld, moved)
        whole, y = guarded(b, c, ld, dtype)
        hip.grouped_cell_fused(x, [(hip.pack_grouped_weights(w, case.groups), bias, k, d) for w, bias, k, d in nodes], case.mask, y, t, case.groups, ln, None)
        torch.cuda.synchronize()
        assert_written(whole, y, t, f'moved tap, {dtype}')
        assert_exact(y, t, want_moved, f'moved tap, {dtype}')
        assert not torch.equal(y[:, :, :t].double().cpu(), want)
