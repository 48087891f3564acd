"""The tile and kernel-variant choosers (nb_asr_amd/tiles.py) are plain arithmetic over (batch, shape) and two measured tables: every
choice is pinned against tests/golden/tile_choices.json, recorded from the ``ForwardPlan`` methods they were before they became free
functions (``_row_tile``, ``_bf16_tile``, ``_dense_tile``, ``_gc_variant``).  No GPU needed."""
import itertools
import json
import pathlib
import types

import pytest

from nb_asr_amd import ops, tiles

GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden' / 'tile_choices.json'
BATCHES = (1, 2, 4, 8, 12, 16, 32, 64, 128)
CONVS = ((80, 600, 1), (600, 800, 1), (800, 1000, 2), (1000, 1200, 2))       # (c_in, c_out, stride) of the model's downsample convolutions
FRAMES_OUT = (77, 125, 250, 500, 999, 1000, 1600)
GC_OPS = tuple(itertools.product((5, 7), (1, 2), (6, 8, 10, 12)))             # (taps, dilation, channels per group)
GC_FLAVOURS = ('lnx', 'lnx+skip', 'skip', 'plain')
GC_SIZES = tuple(itertools.product((2, 8, 64), (250, 1000)))                  # (utterances, frames)
GC_FORCED = (None, '0', '12')                                                 # NBASR_GC_F32_VARIANT
GROUPS = 100


def tile_cases():
    """(key, batch, (c_in, c_out, stride), frames_out)"""
    for batch, conv, frames_out in itertools.product(BATCHES, CONVS, FRAMES_OUT):
        yield f'{batch}|{conv[0]},{conv[1]},{conv[2]}|{frames_out}', batch, conv, frames_out


def gc_node(taps, dilation, flavour):
    """A stand-in for a cell node as the chooser reads it, and the (ln0, n_inputs) of a launch of that flavour."""
    skip = ops.Identity() if 'skip' in flavour else ops.Zero()
    on_x = flavour.startswith('lnx')
    node = types.SimpleNamespace(op=types.SimpleNamespace(kernel_size=taps, dilation=dilation, groups=GROUPS),
                                 branch_ops=[skip] if on_x else [skip, ops.Zero()])
    return node, (('stats', 'gamma', 'beta'), 1) if on_x else (None, 2)


def gc_cases():
    """(key, forced, shape, node, ln0, stats, n_inputs)"""
    for (taps, dilation, cg), flavour, with_stats, (batch, frames), forced in itertools.product(GC_OPS, GC_FLAVOURS, (False, True), GC_SIZES, GC_FORCED):
        node, (ln0, n_inputs) = gc_node(taps, dilation, flavour)
        key = f'{taps},{dilation},{cg}|{flavour}|{"stats" if with_stats else "-"}|{batch}x{frames}|{forced}'
        yield key, forced, (batch, cg * GROUPS, (frames + 3) & ~3), node, ln0, ('stats_out', 'ws', 1e-3) if with_stats else None, n_inputs


@pytest.fixture(scope='module')
def recorded():
    return json.loads(GOLDEN.read_text())


def test_tile_choices_are_the_recorded_ones(recorded, monkeypatch):
    monkeypatch.delenv('NBASR_BF16_FTILE', raising=False)
    want, n = recorded['tiles'], 0
    for key, batch, (c_in, c_out, stride), frames_out in tile_cases():
        got = [tiles.row_tile(batch, c_out, frames_out), tiles.row_tile(batch, c_out, frames_out, allow_64=False),
               list(tiles.dense_tile(batch, c_in, c_out, stride, frames_out)),
               list(tiles.bf16_tile(batch, c_out, frames_out)), list(tiles.bf16_tile(batch, c_out, frames_out, pipe=True))]
        assert got == want[key], key
        n += 1
    assert n == len(want) == len(BATCHES) * len(CONVS) * len(FRAMES_OUT)


def test_variant_choices_are_the_recorded_ones(recorded, monkeypatch):
    want, n = recorded['gc_variant'], 0
    for key, forced, shape, node, ln0, stats, n_inputs in gc_cases():
        if forced is None:
            monkeypatch.delenv('NBASR_GC_F32_VARIANT', raising=False)
        else:
            monkeypatch.setenv('NBASR_GC_F32_VARIANT', forced)
        assert tiles.gc_variant(tiles._GC_TABLE, shape, node, ln0, stats, n_inputs) == want[key], key
        n += 1
    assert n == len(want) == len(GC_OPS) * len(GC_FLAVOURS) * 2 * len(GC_SIZES) * len(GC_FORCED)
    assert len(set(want.values())) > 3                    # (the table's choices, the default kernel and the forced variant all occur)


def test_every_tiling_the_planner_can_pick_is_exercised_on_the_gpu(monkeypatch):
    """Closure: whatever ``dense_tile`` and ``bf16_tile`` (plain and pipelined) return for 1 ... 128 utterances of 40 ... 3000 frames through
    the model's four convolutions is an instantiation that tests/test_dense_tilings_gpu.py runs element by element (dense_tilings.EXERCISED)
    -- the fp16 image path, which always emits the statistics by-product, with it.  A tiling added to tiles.py fails here, without a
    GPU, until a GPU test names it."""
    import dense_tilings as dt
    monkeypatch.delenv('NBASR_BF16_FTILE', raising=False)
    picked = set()
    for batch, frames in itertools.product(range(1, 129), range(40, 3001, 20)):
        t = frames
        for c_in, c_out, stride in CONVS:
            t = (t + stride - 1) // stride                          # frames out of this convolution, into the next
            picked.add((dt.F16_IMAGE, stride, *tiles.dense_tile(batch, c_in, c_out, stride, t)))
            picked.add((dt.BF16, stride, *tiles.bf16_tile(batch, c_out, t)))
            picked.add((dt.BF16, stride, *tiles.bf16_tile(batch, c_out, t, pipe=True)))
    for scheme, stride, rows, frame_tile in sorted(picked):
        assert (scheme, stride, rows, frame_tile, False) in dt.EXERCISED, (scheme, stride, rows, frame_tile)
        if scheme == dt.F16_IMAGE:
            assert (scheme, stride, rows, frame_tile, True) in dt.EXERCISED, (scheme, stride, rows, frame_tile, 'statistics')
    # the enumeration is not vacuous: it reaches the 512-frame bf16 tiles at both strides and row tiles, and 128-frame fp16 tiles
    bf16 = {p[1:] for p in picked if p[0] == dt.BF16}
    f16 = {p[1:] for p in picked if p[0] == dt.F16_IMAGE}
    assert {(s, rows, 512) for s in (1, 2) for rows in (128, 160)} <= bf16
    assert any(ft == 128 for _, _, ft in f16) and {rows for _, rows, _ in f16} == set(dt.F16_IMAGE_ROWS)
    # every GPU case is drawn from EXERCISED, and every EXERCISED entry has a case at its stride
    assert {(dt.BF16, shape[3], rows, ft, False) for shape, rows in dt.bf16_cases() for r, ft in dt.tilings(dt.BF16, shape[3], False) if r == rows} \
        == {e for e in dt.EXERCISED if e[0] == dt.BF16}
    assert {(dt.F16_IMAGE, shape[3], rows, ft, True) for shape, rows, ft in dt.stats_cases()} == {e for e in dt.EXERCISED if e[0] == dt.F16_IMAGE and e[4]}
    ran = {(scheme, shape[3], *tile, True) for shape, route in dt.route_cases() for scheme, tile in dt.ROUTES[route]}
    assert {e for e in dt.EXERCISED if e[0] in (dt.F16_SPLIT, dt.BF16X3) and e[4]} <= ran <= dt.EXERCISED
    assert len(dt.route_cases()) == len(dt.ROUTE_SHAPES) * len(dt.ROUTES)


def test_dense_tile_rule_and_measured_table():
    """The whole-rounds model at 2, 8 and 64 utterances, and the measured table (dense_tile_table.json) that overrules it where it knows the
    shape (round 5): 128-frame tiles for the stride-2 convs of a small batch, 64-row tiles (two workgroups per CU) for conv 0; shapes it does
    not know keep the model's choice.  The layers are those of a real model."""
    import cases
    import nb_asr_amd as nb
    model = nb.get_model(cases.ARCH_A, use_rnn=True, dropout_rate=0.0)
    convs = [(l.conv.in_channels, l.conv.out_channels, l.strides) for l in model.model if hasattr(l, 'conv') and getattr(l, 'strides', 0)]
    assert tuple(convs) == CONVS
    c0, c1, c2, c3 = convs
    batch = 2
    assert tiles.row_tile(batch, 800, 1000) == 64 and tiles.row_tile(batch, 1200, 250) == 64      # 2 utterances: under one round, so the smallest tiles
    batch = 64
    assert (tiles.row_tile(batch, 800, 1000) == 160 and tiles.row_tile(batch, 1000, 500) == 128 and tiles.row_tile(batch, 1200, 250) == 160
            and tiles.row_tile(batch, 600, 1000) == 128)
    batch = 8
    assert tiles.row_tile(batch, 1000, 500) == 64 and tiles.row_tile(batch, 1200, 250) == 64 and tiles.row_tile(batch, 800, 1000) == 128

    def within_3_percent_of_the_tables_best(conv, frames_out, key):
        row = tiles._DENSE_TILES[key][batch]
        return row[tiles.dense_tile(batch, *conv, frames_out)] <= min(row.values()) / 0.97
    assert tiles.dense_tile(batch, *c3, 250) == (64, 128) and tiles.dense_tile(batch, *c3, 77) == (tiles.row_tile(batch, 1200, 77), 256)
    assert within_3_percent_of_the_tables_best(c2, 500, (800, 1000, 2, 500)) and within_3_percent_of_the_tables_best(c0, 1000, (80, 600, 1, 1000))
    batch = 64
    assert tiles.dense_tile(batch, *c0, 1000) == (64, 256) and tiles.dense_tile(batch, *c2, 500) == (128, 256) and tiles.dense_tile(batch, *c3, 250) == (160, 256)
    assert within_3_percent_of_the_tables_best(c1, 1000, (600, 800, 1, 1000))
