"""The tilings and routes of the k = 8 downsample convolution that a GPU test runs element by element, and the shapes it runs them at.

``nb_asr_amd/tiles.py`` picks a (row tile, frame tile) per launch from the batch and the frame count; every one is a kernel
instantiation of its own (``gemm_conv_split.hip``).  EXERCISED names the instantiations that ``tests/test_dense_tilings_gpu.py`` is
parametrised over; ``tests/test_tiles_host.py`` enumerates what the planner can return and fails -- without a GPU -- when it returns one
that is not named here.  A new tiling in ``tiles.py`` therefore needs an entry here, and with the entry comes its GPU test.

Plain data: no GPU, no fixtures, no imports from the package.
"""
import itertools

# scheme names as ``ForwardPlan.dense_schemes`` records them
F16_IMAGE, BF16, F16_SPLIT, BF16X3 = 'f16x2-image', 'bf16', 'f16x2', 'bf16x3'

F16_IMAGE_ROWS, F16_IMAGE_FRAMES = (64, 96, 128, 160), (128, 256)
BF16_ROWS, BF16_FRAMES = (128, 160), (256, 512)
REFERENCE_TILE = (128, 256)               # the tiling every other one is compared with, bit for bit

# (scheme, stride, rows, frame_tile, with_stats)
EXERCISED = frozenset(
    # one-term bf16 GEMM on nbasr_bf16_image's operand (it has no statistics by-product)
    [(BF16, s, rows, ft, False) for s, rows, ft in itertools.product((1, 2), BF16_ROWS, BF16_FRAMES)]
    # fp16-split GEMM on the pre-split image: y without and with the statistics by-product
    + [(F16_IMAGE, s, rows, ft, st) for s, rows, ft, st in itertools.product((1, 2), F16_IMAGE_ROWS, F16_IMAGE_FRAMES, (False, True))]
    # the kernels that split their operand in the prologue: one tiling each
    + [(scheme, s, *REFERENCE_TILE, st) for scheme, s, st in itertools.product((F16_SPLIT, BF16X3), (1, 2), (False, True))])

# ---- one-term bf16 GEMM: (c_in, c_out, frames_in, stride, batch), the smallest shapes that reach each edge of the 512-frame tile ----
BF16_SHAPES = (
    (24, 40, 1, 1, 2),            # one frame
    (24, 136, 513, 1, 3),         # second frame tile with one live frame; 1.5 channel groups; second row tile of 8 rows; the id decodes 3 utterances
    (40, 161, 1031, 2, 2),        # stride 2 with odd input length; 516 output frames; 2.5 groups; 161 = 160 + 1 rows
    (8, 40, 1024, 2, 2),          # exactly one full 512-frame tile; half a channel group
    (136, 200, 640, 1, 2),        # the second tile holds exactly one wave's 128 frames
    (72, 129, 383, 1, 2),         # third wave column one frame short; row tile of one row
    (1000, 1200, 130, 2, 2),      # production K depth of 63 groups; 10 / 8 row tiles
)

# ---- statistics by-product on the fp16 image path: (c_in, c_out, frames_in, stride, batch) ----
STATS_SHAPES = (
    (24, 40, 1, 1, 1),
    (48, 200, 75, 2, 2),
    (32, 161, 130, 1, 2),
    (40, 136, 259, 1, 3),         # crosses a 128-frame and a 256-frame tile
)

# ---- statistics by-product on the other routes ----
ROUTE_SHAPES = (
    (48, 200, 75, 2, 3),
    (32, 161, 130, 1, 3),
)
# route -> the EXERCISED schemes its launches run: (scheme, (rows, frame_tile)) per leg
ROUTES = {
    'f16x2+absmax': ((F16_SPLIT, REFERENCE_TILE),),
    'bf16x3': ((BF16X3, REFERENCE_TILE),),
    'bf16x3+deferred-ln': ((BF16X3, REFERENCE_TILE),),
    'first-ranged': ((F16_SPLIT, REFERENCE_TILE), (BF16X3, REFERENCE_TILE)),
    'first-ranged+image': ((F16_IMAGE, REFERENCE_TILE), (BF16X3, REFERENCE_TILE)),
    'first-ranged+image-64x128': ((F16_IMAGE, (64, 128)), (BF16X3, REFERENCE_TILE)),
}


def tilings(scheme, stride, with_stats):
    """The (rows, frame_tile) pairs EXERCISED holds for a scheme at a stride, sorted."""
    return sorted({(rows, ft) for sch, s, rows, ft, st in EXERCISED if (sch, s, st) == (scheme, stride, with_stats)})


def bf16_cases():
    """(shape, rows): every bf16 shape at every row tile EXERCISED names for its stride; the test runs all of that row tile's frame tiles."""
    return [(shape, rows) for shape in BF16_SHAPES for rows in sorted({r for r, _ in tilings(BF16, shape[3], False)})]


def stats_cases():
    """(shape, rows, frame_tile): every statistics shape at every fp16 image tiling EXERCISED names for its stride."""
    return [(shape, rows, ft) for shape in STATS_SHAPES for rows, ft in tilings(F16_IMAGE, shape[3], True)]


def route_cases():
    """(shape, route) for which every leg of the route is in EXERCISED with the statistics by-product."""
    return [(shape, route) for shape in ROUTE_SHAPES for route, legs in ROUTES.items()
            if all((scheme, shape[3], *tile, True) in EXERCISED for scheme, tile in legs)]
