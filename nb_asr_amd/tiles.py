"""Tile and kernel-variant choices of the forward: plain arithmetic over (batch, shape) and two measured tables.

Every choice here is speed only -- each tiling and each variant computes the same sums in the same order --, so these are free functions
that own nothing: ``walk.py`` calls them with ``plan.batch``, and a test needs no plan and no device.  NBASR_GC_F32_VARIANT and
NBASR_BF16_FTILE are read at every call, here and nowhere else.
"""
import math
import os

import torch

from . import hip


def _load_gc_table():
    import json
    import pathlib
    path = pathlib.Path(__file__).with_name('gc_variant_table.json')
    return json.loads(path.read_text()) if path.exists() else {}


_GC_TABLE = _load_gc_table()


def _load_dense_tile_table():
    """Measured us per launch of the image-path dense convolution per (row tile, frame tile): nb_asr_amd/dense_tile_table.json
    (tools/ubench/dense_tiles.py -> tools/make_dense_tile_table.py), {(c_in, c_out, stride, frames_out): {batch: {(rows, frames): us}}}."""
    import json
    import pathlib
    path = pathlib.Path(__file__).with_name('dense_tile_table.json')
    if not path.exists():
        return {}
    raw = json.loads(path.read_text())['table']
    return {tuple(int(v) for v in k.split(',')): {int(b): {tuple(int(v) for v in t.split('x')): us for t, us in row.items()} for b, row in by_b.items()}
            for k, by_b in raw.items()}


_DENSE_TILES = _load_dense_tile_table()


def row_tile(batch, c_out, frames_out, allow_64=True):
    """Rows per workgroup of the image-path GEMM: 128, or 160 where that means less work in whole rounds of workgroups
    (a tile's cost is proportional to its rows; 256 CUs run one workgroup each).  At the benchmark shape: 160 for
    C_out = 800 (5 full row tiles instead of 7 with the last a quarter full) and 1200 (512 workgroups instead of 640)."""
    n_nt = (hip.round_up4(frames_out) + 255) // 256

    def cost(rows):
        wgs = -(-c_out // rows) * n_nt * batch
        return -(-wgs // 256) * rows
    rows = 160 if cost(160) < cost(128) else 128
    # smaller tiles where a small batch leaves CUs without a workgroup (8 utterances: 128 or 80 workgroups for convs 2 and 3).  A
    # smaller tile does less per operand byte staged, so it has to win by a margin: 96 rows (round 4: 13 x 16 = 208 workgroups in ONE
    # round for conv 3 at 16 utterances) by a tenth, 64 rows by a quarter (measured +4 % at 8 utterances, nothing to gain at 32)
    score = float(cost(rows))
    if allow_64:
        for r, margin in ((96, 1.1), (64, 1.25)):
            if margin * cost(r) < score:
                rows, score = r, margin * cost(r)
    return rows


def bf16_tile(batch, c_out, frames_out, pipe=False):
    """(rows, frames) per workgroup of the one-term bf16 GEMM: rows 128 / 160, frames 256 / 512 (results are bit-identical, the choice
    is speed only).  That flavour is bound by LDS reads; a 512-frame tile re-uses a weight fragment 8 times instead of 4 and runs
    its K-steps ~10 % faster per unit of work (measured at 32 x 1600: conv 2 312 -> 283 us, conv 3 237 -> 213) -- where the frames
    and the workgroup count still fill whole tiles and rounds (conv 1, 1600 frames = 3.1 tiles of 512: 357 -> 362).  Cost = rounds
    of 256 workgroups x tile area x that factor.  In a PIPELINED forward the 256-frame tiles stay: the wide tiles' workgroups (237-245
    registers, twice as long-lived) leave the per-frame launches of the previous batch's LSTM tail waiting for a compute unit --
    dense convs 0.983 -> 0.924 ms per forward but 9 620 -> 9 190 utterances/s (three alternating same-box runs each)."""
    forced = os.environ.get('NBASR_BF16_FTILE')
    best = None
    for rows in (128, 160):
        for ftile in ((int(forced),) if forced else (256,) if pipe else (256, 512)):
            wgs = -(-c_out // rows) * -(-hip.row_pitch(frames_out, torch.bfloat16) // ftile) * batch
            cost = -(-wgs // 256) * rows * ftile * (0.9 if ftile == 512 else 1.0)
            if best is None or cost < best[0]:
                best = (cost, rows, ftile)
    return best[1], best[2]


def dense_tile(batch, c_in, c_out, stride, frames_out):
    """(row tile, frame tile) of the image-path fp16 GEMM for this launch.  Every tiling computes the same sums in the same order
    (results are bit-identical), so the choice is speed only: `row_tile`'s whole-rounds model, overruled by the measured table
    (dense_tile_table.json: every tiling at 4 ... 64 utterances x 1000 frames) where that knows the shape and a tiling beat the
    model's choice by more than 3 % -- 128-frame tiles and 64-row tiles at small batches (one round of workgroups: conv 3 at 8
    utterances 185 -> 168 us), 64-row tiles for conv 0 at every batch (two workgroups per CU: its ten K-steps are mostly prologue
    and epilogue)."""
    rows = row_tile(batch, c_out, frames_out)
    best = (rows, 256)
    for (ci_ref, co_ref, s_ref, t_ref), by_batch in _DENSE_TILES.items():
        if (ci_ref, co_ref, s_ref) != (c_in, c_out, stride) or not 0.75 * t_ref <= frames_out <= 1.34 * t_ref:
            continue
        b_ref = min(by_batch, key=lambda b: abs(math.log2(max(batch, 1) / b)))
        if not 0.7 * b_ref <= batch <= 1.42 * b_ref:
            break
        row = by_batch[b_ref]
        cand = min(row, key=row.get)
        if row[cand] < 0.97 * row.get(best, float('inf')):
            best = cand
        break
    return best


def gc_variant(table, shape, node=None, ln0=None, stats=None, n_inputs=0):
    """Kernel variant of the fp32 grouped-conv node op for this launch (speed only: every variant computes the same sums in the
    same order, results are bit-identical).  NBASR_GC_F32_VARIANT=<int> forces one (diagnostics; needs ld % 8 == 0 for the
    8-frame variants; the output-split ones are never forced onto a statistics launch, which they do not have).

    Default: looked up in gc_variant_table.json, which tools/make_gc_variant_table.py derives from same-process A/B timings of
    the variants {default, output split, pipelined buffer loads, both, LDS ring, persistent LDS ring} per (taps, dilation,
    channels per group, flavour, size class) on an MI355X (tools/ubench/ab_gc_variants.py, profiles/r03_gc_variants/)."""
    forced = os.environ.get('NBASR_GC_F32_VARIANT')
    if forced is not None:
        v = int(forced)
        return (v & ~hip.GC_OSPLIT if v & hip.GC_PIPE else 0) if (v & hip.GC_OSPLIT and (stats is not None or node is None)) else v
    if node is None or not table:
        return 0
    op = node.op
    groups = getattr(op, 'groups', 0)
    if not groups:
        return 0
    b, c, ld = shape
    waves_per_simd = b * groups * (-(-(ld // 4) // 64)) / 1024.0
    on_x = ln0 is not None and n_inputs == 1
    has_skips = any(type(br).__name__ == 'Identity' for br in node.branch_ops)
    flavour = ('lnx+skip' if has_skips else 'lnx') if on_x else ('skip' if has_skips else 'plain')
    head = f"{op.kernel_size},{op.dilation},{c // groups},"
    tail = f",{'small' if waves_per_simd < 4.0 else 'large'}{',stats' if stats is not None else ''}"
    v = table.get(head + flavour + tail)
    if v is None and on_x:                           # (tables older than round 3 have one LayerNorm-on-load class)
        v = table.get(head + 'lnx' + tail)
    return v or 0
