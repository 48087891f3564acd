"""Every tiling and statistics route of the k = 8 downsample convolution that ``nb_asr_amd/tiles.py`` can pick, element by element.

``tiles.py`` promises that a tiling decides which workgroup computes an output, never the order of its sums.  The instantiations are
listed in ``tests/dense_tilings.py`` (EXERCISED); ``tests/test_tiles_host.py`` checks without a GPU that the planner returns no other.

* the one-term bf16 GEMM at 256- and 512-frame tiles, 128 and 160 rows: the same bits, an fp64 oracle with a derived bound, and every
  byte of the pitched output written exactly once inside its allocation;
* a bf16 model forced to either frame tile: the same logits, bit for bit;
* the statistics by-product (``stats_part``) on all eight tilings of the fp16 image path and on the routes that split their operand
  in the kernel, the two-leg first convolution included: y untouched, every live partial written, the merged statistics as close to
  fp64 as a statistics pass over y.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import cases
import dense_tilings as dt
import nb_asr_amd as nb
from nb_asr_amd import hip
from nb_asr_amd.weights import keyed_fill_, keyed_input
from oracle import asr_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF = torch.bfloat16
NAN = float('nan')
GUARD = 64                      # bf16 elements on either side of y: 128 bytes, y stays 16-byte aligned


# ---- B. the one-term bf16 GEMM ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bf16_operands(shape):
    """bf16-valued fp32 operands on the CPU, one draw per shape (shared by every row tile and both operand flavours)."""
    c_in, c_out, t, stride, b = shape
    torch.manual_seed(c_in + t)
    x = torch.randn(b, c_in, t).to(BF).float()
    w = (torch.randn(c_out, c_in, 8) * (2.0 / (c_in * 8)) ** 0.5).to(BF).float()
    bias = (torch.randn(c_out) * 0.2).to(BF).float()
    gamma, beta = torch.rand(c_in) * 0.4 + 0.8, torch.randn(c_in) * 0.1
    return x, w, bias, gamma, beta


@functools.lru_cache(maxsize=None)
def bf16_reference(shape):
    """(want, tol, cpu): the fp64 evaluation of PadConvRelu on the bf16-valued operands, the tolerance

        |got - want| <= 2^-8 |want| + (8 c_in + 1) 2^-23 pre,      pre = sum |w| |x| + |b|  (fp64, the same left padding, NOT clamped)

    -- one bf16 round-to-nearest of the result (8 significand bits: half a step is at most 2^-8 of the value) plus the standard bound of
    an fp32 sum of 8 c_in exact products and the bias, u = 2^-24 per addition, doubled for the matrix core's internal order; ReLU and the
    clamp at 20 are 1-Lipschitz, so the bound survives them -- and the CPU's own fp32 evaluation rounded once to bf16."""
    c_in, c_out, t, stride, b = shape
    x, w, bias, _, _ = bf16_operands(shape)
    want = oracle.pad_conv_relu(x.double(), w.double(), bias.double(), 1, stride, 1)
    lpad, rpad = oracle.pad_amounts(8, 1, stride)
    pre = F.conv1d(F.pad(x.double().abs(), (lpad, rpad)), w.double().abs(), bias.double().abs(), stride=stride)
    tol = 2.0 ** -8 * want.abs() + (8 * c_in + 1) * 2.0 ** -23 * pre
    cpu = oracle.pad_conv_relu(x, w, bias, 1, stride, 1).to(BF).double()
    return want, tol, cpu


@functools.lru_cache(maxsize=None)
def bf16_reference_normed(shape):
    """The existing image-path test's reference with the LayerNorm written into the image: fp32 on the bf16-rounded normalised operand."""
    x, w, bias, gamma, beta = bf16_operands(shape)
    xin16 = oracle.layer_norm_channels(x, gamma, beta).to(BF).float()
    return oracle.pad_conv_relu(xin16, w, bias, 1, shape[3], 1)


def bf16_launch(shape, rows, frame_tile, with_norm):
    """One launch into the middle of a NaN-filled allocation: (the whole allocation, y as a view of its middle)."""
    c_in, c_out, t, stride, b = shape
    x, w, bias, gamma, beta = bf16_operands(shape)
    t_out = (t + stride - 1) // stride
    ld, ld_out = hip.row_pitch(t, BF), hip.row_pitch(t_out, BF)
    xp = torch.zeros(b, c_in, ld, dtype=BF, device=DEV)
    xp[:, :, :t] = x.to(BF)
    image = torch.full((hip.bf16_image_bytes(b, c_in, ld),), 0x7f, dtype=torch.uint8, device=DEV)     # poison: every row the conv reads must have been written
    stats = torch.empty(b, 2, ld, device=DEV)
    hip.bf16_image(xp, image, t, (gamma.to(DEV), beta.to(DEV)) if with_norm else None, stats if with_norm else None, 1e-3)
    packed = hip.pack_dense_weights_bf16(w.to(DEV), stride, rows)
    n = b * c_out * ld_out
    whole = torch.full((n + 2 * GUARD,), NAN, dtype=BF, device=DEV)
    y = whole[GUARD:GUARD + n].view(b, c_out, ld_out)
    hip.dense_conv1d_bf16_img(image, b, c_in, t, ld, packed, c_out, 8, bias.to(DEV), y, stride, rows, frame_tile)
    torch.cuda.synchronize()
    return whole, y


def test_the_bf16_tolerance_is_neither_vacuous_nor_too_tight():
    """The bound of ``bf16_reference`` against the CPU's own fp32 evaluation, rounded once to bf16, at every shape: inside it (the bound is
    a theorem for that evaluation too), and using at least a tenth of it -- so an edit of the shapes or of the bound cannot quietly loosen
    the GPU comparison.  The rounding of the result alone reaches the first term at the bottom of a binade; the summation term is a worst
    case that grows with K and that no evaluation comes near, which is what separates the production depth (0.21 at c_in = 1000) from
    the shallow shapes (0.80 ... 0.99)."""
    for shape in dt.BF16_SHAPES:
        want, tol, cpu = bf16_reference(shape)
        ratio = float(((cpu - want).abs() / tol.clamp_min(1e-300)).max())
        print(f'{shape}: CPU fp32 -> bf16 reaches {ratio:.3f} of the tolerance')
        assert 0.1 <= ratio <= 1.0, (shape, ratio)


@pytest.mark.parametrize('with_norm', [False, True])
@pytest.mark.parametrize('shape,rows', dt.bf16_cases())
def test_bf16_frame_tiles_are_bit_identical_and_match_fp64(shape, rows, with_norm):
    """image (plain re-layout, or LayerNorm written as the operand) -> one-term bf16 GEMM at every frame tile of this row tile.
    Measured on an MI355X against the fp64 bound: 0.85, 0.96, 0.93, 0.99, 0.80, 0.88 and 0.21 of it at the seven shapes, the same at
    every tiling and the same as the CPU's fp32 evaluation reaches (the worst element is the one rounding of the result)."""
    c_in, c_out, t, stride, b = shape
    t_out = (t + stride - 1) // stride
    frame_tiles = [ft for r, ft in dt.tilings(dt.BF16, stride, False) if r == rows]
    assert dt.REFERENCE_TILE[1] in frame_tiles and len(frame_tiles) > 1
    outs = {}
    for ft in frame_tiles:
        whole, y = bf16_launch(shape, rows, ft, with_norm)
        # every element of y was written, pitch columns with zeros, and nothing outside y
        assert bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[-GUARD:]).all()), ft
        assert bool(torch.isfinite(y[:, :, :t_out].float()).all()), ft
        assert bool((y[:, :, t_out:] == 0).all()), ft
        outs[ft] = y
    ref = outs[dt.REFERENCE_TILE[1]]
    for ft, y in outs.items():
        assert torch.equal(y, ref), (ft, float((y.float() - ref.float()).abs().max()))       # tiles.bf16_tile: "results are bit-identical"
    for ft, y in outs.items():
        got = y[:, :, :t_out].float().cpu()
        if with_norm:
            # the LayerNorm'd operand can round differently by one bf16 step where the fp32 value sits on a rounding boundary: the
            # existing image-path test's criterion; the bit identity to the 256-frame tile carries the precision
            want = bf16_reference_normed(shape)
            tol = 2.0 ** -8 * want.abs() + 3e-2
            assert bool(((got - want).abs() <= tol).all()), (ft, float(((got - want).abs() / tol).max()))
            assert float((got - want).abs().mean()) <= 2.0 ** -9 * float(want.abs().mean()) + 2e-3, ft
        else:
            want, tol, _ = bf16_reference(shape)
            ratio = float(((got.double() - want).abs() / tol.clamp_min(1e-300)).max())
            print(f'{shape} rows {rows} frame tile {ft}: worst |got - want| / tolerance = {ratio:.3f}')
            assert ratio <= 1.0, (ft, ratio)


def test_bf16_scheme_refuses_the_tilings_it_does_not_have():
    shape = dt.BF16_SHAPES[0]
    c_in, c_out, t, stride, b = shape
    _, w, bias, _, _ = bf16_operands(shape)
    ld = hip.row_pitch(t, BF)
    xp = torch.zeros(b, c_in, ld, dtype=BF, device=DEV)
    image = hip.bf16_image(xp, torch.empty(hip.bf16_image_bytes(b, c_in, ld), dtype=torch.uint8, device=DEV), t)
    y = torch.zeros(b, c_out, hip.row_pitch(t, BF), dtype=BF, device=DEV)
    packed = hip.pack_dense_weights_bf16(w.to(DEV), stride)
    for ft in (128, 64):
        with pytest.raises(hip.HipError, match='256- and 512-frame tiles'):
            hip.dense_conv1d_bf16_img(image, b, c_in, t, ld, packed, c_out, 8, bias.to(DEV), y, stride, 128, ft)
    packed96 = hip.pack_dense_weights_bf16(w.to(DEV), stride, 96)
    with pytest.raises(hip.HipError, match='row_tile=96'):
        hip.dense_conv1d_bf16_img(image, b, c_in, t, ld, packed96, c_out, 8, bias.to(DEV), y, stride, 96)
    torch.cuda.synchronize()
    assert bool((y == 0).all())                                   # a refused launch wrote nothing


# ---- C. the model: a forced frame tile changes no bit ---------------------------------------------------------------------------------
def test_bf16_model_logits_do_not_depend_on_the_frame_tile(monkeypatch):
    """ARCH_D in bf16 at 2 x 1040 frames: the four convolutions write 1040, 1040, 520 and 260 frames -- three ragged 512-frame tiles, two,
    and one.  NBASR_BF16_FTILE forces either tile on all four; the logits are the same bits."""
    m = nb.get_model(cases.ARCH_D, use_rnn=True, dropout_rate=0.0)
    keyed_fill_(m, seed=1235, mode='lively')
    m = m.to(DEV).to(BF).eval()
    x = keyed_input(2, 1040, seed=0).to(BF).to(DEV)
    logits = {}
    for forced in (256, 512):
        monkeypatch.setenv('NBASR_BF16_FTILE', str(forced))
        m._plans.clear()
        with torch.no_grad():
            logits[forced] = m(x).clone()
        plan = m._plans.values()[-1]
        assert set(plan.dense_schemes.values()) == {dt.BF16} and set(plan.dense_frame_tiles) == {0, 1, 2, 3}
        assert set(plan.dense_frame_tiles.values()) == {forced}
        assert all((dt.BF16, s, plan.dense_row_tiles[blk], forced, False) in dt.EXERCISED for blk, s in enumerate((1, 1, 2, 2)))
    assert bool(torch.isfinite(logits[256].float()).all())
    assert torch.equal(logits[512], logits[256])


# ---- D. the statistics by-product ---------------------------------------------------------------------------------------------------
def pitched(x):
    b, c, t = x.shape
    buf = torch.zeros(b, c, hip.round_up4(t), device=DEV)
    buf[:, :, :t] = x.to(DEV)
    return buf


def statistics_errors(y, t_out, got):
    """Relative errors (mean, rstd) of the merged statistics ``got`` and of a statistics pass over y, both against the fp64 statistics
    of that y -- the criterion of test_dense_conv_emits_the_statistics_of_its_output: e_got <= max(4 e_ref, 1e-6)."""
    b, _, ld_out = y.shape
    want = torch.empty(b, 2, ld_out, device=DEV)
    hip.channel_stats(y, want, t_out, 1e-3)
    y64 = y[:, :, :t_out].double().cpu()
    mean64, var64 = y64.mean(dim=1), y64.var(dim=1, unbiased=False)
    rstd64 = 1.0 / (var64 + 1e-3).sqrt()
    errors = {}
    for name, col, truth in (('mean', 0, mean64), ('rstd', 1, rstd64)):
        e_got = float((got[:, col, :t_out].double().cpu() - truth).abs().max() / truth.abs().max())
        e_ref = float((want[:, col, :t_out].double().cpu() - truth).abs().max() / truth.abs().max())
        errors[name] = (e_got, e_ref)
    return errors


def assert_statistics(y, t_out, part, c_out, label):
    """The partials of one launch: every live one written, and their merge as close to fp64 as a pass over y; pitch columns zero."""
    b, _, ld_out = y.shape
    live = part.view(-1, b, 2, ld_out)[..., :t_out]
    assert live.shape[0] == -(-c_out // hip.DENSE_STATS_UNIT)
    assert bool(torch.isfinite(live).all()), (label, 'a live partial was not written')
    got = torch.full((b, 2, ld_out), NAN, device=DEV)
    hip.grouped_stats_finalize(part, got, c_out, t_out, c_out, 1e-3, hip.DENSE_STATS_UNIT)
    assert bool((got[:, :, t_out:] == 0).all()), label
    for name, (e_got, e_ref) in statistics_errors(y, t_out, got).items():
        assert e_got <= max(4.0 * e_ref, 1e-6), (label, name, e_got, e_ref)


def conv_weights(c, c_out, seed):
    torch.manual_seed(seed)
    w, bias = torch.randn(c_out, c, 8) * (2.0 / (c * 8)) ** 0.5, torch.randn(c_out) * 0.3
    bias[: c_out // 3] -= 30.0                                    # a third of the channels sit at exactly 0 behind the ReLU
    return w.to(DEV), bias.to(DEV)


@functools.lru_cache(maxsize=None)
def image_stats_reference(shape):
    """The operands of one statistics shape on the device and the (128, 256) launch every other tiling is compared with."""
    c, c_out, t, stride, b = shape
    w, bias = conv_weights(c, c_out, c_out + t)
    x = torch.randn(b, c, t) * 1.5 + 0.2
    g, be = torch.rand(c) + 0.5, torch.randn(c) * 0.2
    xp = pitched(x)
    ld = xp.shape[2]
    stats_in, bound = torch.empty(b, 2, ld, device=DEV), torch.empty(b, device=DEV)
    image = hip.split_image(b, c, ld, DEV)
    image.fill_(0x7f)
    hip.layernorm_split_image(xp, g.to(DEV), be.to(DEV), stats_in, bound, image, t, 1e-3)
    t_out = (t + stride - 1) // stride
    ld_out = hip.round_up4(t_out)
    rows, ft = dt.REFERENCE_TILE
    y = torch.full((b, c_out, ld_out), NAN, device=DEV)
    part = torch.full((hip.dense_stats_part_floats(b, c_out, ld_out),), NAN, device=DEV)
    hip.dense_conv1d_fused_packed_f16_img(image, bound, b, c, t, ld, hip.pack_dense_weights(w, stride, 'f16x2', row_tile=rows), c_out, 8, bias, y,
                                          stride, row_tile=rows, stats_part=part, frame_tile=ft)
    torch.cuda.synchronize()
    return dict(image=image, bound=bound, w=w, bias=bias, ld=ld, t_out=t_out, ld_out=ld_out, y=y, part=part)


@pytest.mark.parametrize('shape,rows,frame_tile', dt.stats_cases())
def test_statistics_by_product_on_every_tiling_of_the_image_path(shape, rows, frame_tile):
    """The 16-channel unit, not the tile, is the granule of the partials: every tiling -- the 128-frame ones take two units side by side
    in the two halves of a wave -- leaves the bits of the (128, 256) launch, in y and in every live partial."""
    c, c_out, t, stride, b = shape
    ref = image_stats_reference(shape)
    t_out, ld_out = ref['t_out'], ref['ld_out']
    packed = hip.pack_dense_weights(ref['w'], stride, 'f16x2', row_tile=rows)
    args = (ref['image'], ref['bound'], b, c, t, ref['ld'], packed, c_out, 8, ref['bias'])
    plain = torch.full((b, c_out, ld_out), NAN, device=DEV)
    withp = torch.full_like(plain, NAN)
    part = torch.full_like(ref['part'], NAN)
    hip.dense_conv1d_fused_packed_f16_img(*args, plain, stride, row_tile=rows, frame_tile=frame_tile)
    hip.dense_conv1d_fused_packed_f16_img(*args, withp, stride, row_tile=rows, stats_part=part, frame_tile=frame_tile)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(plain[:, :, :t_out]).all()) and bool((plain[:, :, t_out:] == 0).all())
    assert torch.equal(withp, plain)                              # the by-product leaves y alone
    assert torch.equal(plain, ref['y'])                           # tiles.dense_tile: "results are bit-identical"
    live = part.view(-1, b, 2, ld_out)[..., :t_out]
    assert bool(torch.isfinite(live).all())
    assert torch.equal(live, ref['part'].view(-1, b, 2, ld_out)[..., :t_out])
    assert_statistics(plain, t_out, part, c_out, (rows, frame_tile))


@pytest.mark.parametrize('shape,route', dt.route_cases())
def test_statistics_by_product_on_the_other_routes(shape, route):
    """stats_part on the kernels that split their operand in the prologue (fp16 split with the range of a LayerNorm's output, 3-way bf16
    split, the same behind a deferred LayerNorm) and on the first convolution's two legs, where the fp16 leg (in the kernel or on the
    image) and the bf16x3 leg each write the partials of their own utterances.  Each route against ITSELF: y unchanged by the by-product,
    every live partial of every utterance written once into a NaN-filled buffer, the merge as close to fp64 as a pass over that y.
    (Across routes y differs in the last bits.)"""
    c, c_out, t, stride, b = shape
    w, bias = conv_weights(c, c_out, c_out + t)
    t_out = (t + stride - 1) // stride
    ld_out = hip.round_up4(t_out)
    if route.startswith('first-ranged'):
        x = torch.zeros(b, c, hip.round_up4(t))
        x[:, :, :t] = torch.randn(b, c, t) * 3.0
        x[1, :, t // 2:t] *= 2.0 ** -30                           # extreme: routed to the bf16x3 leg
        x[b - 1] *= 2.0 ** -35                                    # uniformly tiny: ordinary
        x = x.to(DEV)
        rng = hip.input_range(x, t, torch.empty(4 * b, device=DEV))
        legs = rng.view(b, 4).cpu()
        extreme = [bool(r[2] != 0 or r[1] < r[0] * 2.0 ** -12) for r in legs]
        assert extreme == [i == 1 for i in range(b)]              # both legs run
        rows, ft = dt.ROUTES[route][0][1]
        image = None
        if 'image' in route:
            image = hip.split_image(b, c, x.shape[2], DEV)
            image.fill_(0x7f)
        p16 = hip.pack_dense_weights(w, stride, 'f16x2', row_tile=rows if image is not None else 128)
        pb = hip.pack_dense_weights(w, stride, 'bf16x3')

        def launch(y, part):
            hip.dense_conv1d_first_ranged(x, t, rng, p16, pb, c_out, 8, bias, y, stride, image, rows, part, ft)
    else:
        xp = pitched(torch.randn(b, c, t) * 1.5 + 0.2)
        g, be = (torch.rand(c) + 0.5).to(DEV), (torch.randn(c) * 0.2).to(DEV)
        if route == 'f16x2+absmax':
            normed, amax = torch.empty_like(xp), torch.empty(b, device=DEV)
            hip.layernorm_channels(xp, g, be, normed, t, 1e-3, amax)
            packed = hip.pack_dense_weights(w, stride, 'f16x2')

            def launch(y, part):
                hip.dense_conv1d_fused_packed(normed, t, packed, c_out, 8, bias, (), y, stride, scheme='f16x2', x_absmax=amax, stats_part=part)
        else:
            ln = None
            if route == 'bf16x3+deferred-ln':
                ln = (hip.channel_stats(xp, torch.empty(b, 2, xp.shape[2], device=DEV), t, 1e-3), g, be)
            else:
                assert route == 'bf16x3'
            packed = hip.pack_dense_weights(w, stride, 'bf16x3')

            def launch(y, part):
                hip.dense_conv1d_fused_packed(xp, t, packed, c_out, 8, bias, (), y, stride, ln, 'bf16x3', None, part)
    plain = torch.full((b, c_out, ld_out), NAN, device=DEV)
    withp = torch.full_like(plain, NAN)
    part = torch.full((hip.dense_stats_part_floats(b, c_out, ld_out),), NAN, device=DEV)
    launch(plain, None)
    launch(withp, part)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(plain[:, :, :t_out]).all()) and bool((plain[:, :, t_out:] == 0).all())
    assert torch.equal(withp, plain)
    assert_statistics(plain, t_out, part, c_out, route)
