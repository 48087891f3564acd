"""tile_statistics and the kernels around it (layernorm.hip) at the edges of their loops, against fp64 and against the numpy fp32
restatement of the documented order (tests/ln_stats_model.py; what that order can deliver is measured in test_ln_stats_host.py).

    channels  1, 3, 15 (row slots without a channel); 16 | 17; 48 | 49 and 64 | 65 (the 4-in-flight loop starts, its tail);
              112 | 113 and 127, 128 | 129 (the 8-in-flight loop starts, its tail); 176 | 177, 240 | 241 (8, then 4, then the tail;
              two rounds of 8); 600, 1200 (the model's widths)
    frames    fp32: 1, 3, 4, 5, 63, 64, 65, 129, 257       a workgroup covers 64 fp32 frames (16 lanes x 4)
              bf16: 1, 7, 8, 9, 127, 128, 129, 257          ... or 128 bf16 frames (16 lanes x 8)
              -- lanes beyond the row that only attend the barriers, a partial chunk, a full workgroup, one more chunk, three workgroups
    batch     3, and every utterance alone

A. statistics against fp64: e_gpu <= max(4 e_model, 1e-6), e_model the error of the uncontracted restatement on the same input.
B. siblings are the same bits; y of layernorm_channels is an fp32 restatement from those statistics.
C. y and stats sit in the middle of NaN-filled allocations; pitch columns 0; NaN in x's pitch columns and a dead chunk change nothing.
D. the absmax by-product.   E. input_range against exact torch.

MEASURED (MI355X), worst e_gpu / e_model of rstd over the channel edges, per family, fp32 | bf16 storage (criterion: 4):
    benign            1.09 | 1.22  (C = 241 | 176)     worst e_gpu 3.4e-7 | 4.2e-7   (C = 1200)
    offset30          1.02 | 1.01  (C = 129 | 176)                 4.3e-6 | 1.2e-6   (C = 3 | 16)
    offset1000        1.00 | 1.00                                  2.2e-4 | 2.0e-5   (C = 3 | 65)
    relu_sparse       1.09 | 1.25  (C = 177 | 129)                 1.2e-5 | 5.9e-6   (C = 1200)
    first16_outliers  1.14 | 1.14  (C = 177 | 240)                 7.7e-6 | 5.7e-6   (C = 1200)
    constant          1.00 | 1.00                                  7.8e-8            (the rounding of eps and of the root)
    mixed_scale       1.02 | 1.28  (C = 128 | 48)                  3.0e-7 | 2.9e-7   (C = 1200)
The error of the mean never differed from the model's: where compared column by column the mean IS the uncontracted model
bit for bit, and rstd is the model with s2 - dm s1 fused in 98 ... 100 % of the columns (the rest 1-2 ulp away, matching a form that also fuses the merge's M2_b + d d X).
y of layernorm_channels was fma((x - mean) rstd, gamma, beta) in all four instantiations at every shape.
Broken by hand, once: `c + 7 * LN_ROWS <= channels` fails A and B at exactly C = 112, 113, 127, 240, 241 and C at 113; without the
`t0 + r >= frames` zeroing B, C and D fail at every C; without the merge's `nb > 0.f` guard nothing fails and nothing can -- a slot
without a channel holds (0, 0, 0), so it adds delta * 0 and delta * delta * 0 to finite statistics: the guard saves work, not a bit.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import ln_stats_model as lm
from nb_asr_amd import hip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, BF16 = torch.float32, torch.bfloat16
NAN, INF = float('nan'), float('inf')
EPS = 1e-3
BATCH = 3
GUARD = 64                       # elements on either side of an output: at least 128 bytes, the output stays 16-byte aligned
FRAMES = {F32: (1, 3, 4, 5, 63, 64, 65, 129, 257), BF16: (1, 7, 8, 9, 127, 128, 129, 257)}
T_MAX = 257
CASES = [(dtype, c) for dtype in (F32, BF16) for c in lm.CHANNEL_EDGES]
IDS = [f'{"bf16" if d == BF16 else "f32"}-{c}' for d, c in CASES]


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
def guarded(shape, dtype=F32):
    """(the whole NaN-filled allocation, a contiguous view of its middle of the given shape)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), NAN, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n].view(shape)


def guards_intact(whole):
    return bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[-GUARD:]).all())


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=8)
def draw(kind, c, dtype):
    """One draw (BATCH, c, T_MAX) per (family, channels, storage type) as fp32 VALUES of the storage type; every frame count is a
    prefix of it (a column's statistics do not depend on its neighbours)."""
    return torch.from_numpy(lm.family(kind, (BATCH, c, T_MAX), 0)).to(dtype).float()


@functools.lru_cache(maxsize=None)
def affine(c):
    g = torch.Generator().manual_seed(c)
    return torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.2


def put(x, dtype, ld=None, pitch=0.0):
    """(b, c, t) cpu fp32 values -> device tensor of the storage type at pitch ``ld``, pitch columns filled with ``pitch``."""
    b, c, t = x.shape
    out = torch.full((b, c, ld or hip.row_pitch(t, dtype)), pitch, dtype=dtype, device=DEV)
    out[:, :, :t] = x.to(dtype).to(DEV)
    return out


def channel_stats(xd, t):
    whole, stats = guarded((xd.shape[0], 2, xd.shape[2]))
    hip.channel_stats(xd, stats, t, EPS)
    torch.cuda.synchronize()
    assert guards_intact(whole), 'channel_stats wrote outside stats'
    out = stats.cpu()
    assert bool((out[:, :, t:] == 0).all()), 'pitch columns of stats are not 0'
    assert bool(torch.isfinite(out).all())
    return out


def split_image(xd, t, g, be):
    """layernorm_split_image -> (stats, bound, image bytes), all on the cpu."""
    b, c, ld = xd.shape
    whole, stats = guarded((b, 2, ld))
    whole_b, bound = guarded((b,))
    image = hip.split_image(b, c, ld, DEV)
    image.fill_(0x7f)
    hip.layernorm_split_image(xd, g.to(DEV), be.to(DEV), stats, bound, image, t, EPS)
    torch.cuda.synchronize()
    assert guards_intact(whole) and guards_intact(whole_b), 'layernorm_split_image wrote outside stats or bound'
    out = stats.cpu()
    assert bool((out[:, :, t:] == 0).all())
    n_groups = (c + 15) // 16
    return out, bound.cpu(), image.cpu()[:b * n_groups * 4 * (ld + 1) * 16].view(torch.float16).view(b, n_groups, 2, 2, ld + 1, 8)


def bf16_image(xd, t, g, be):
    """bf16_image with a norm -> (stats, image) on the cpu."""
    b, c, ld = xd.shape
    whole, stats = guarded((b, 2, ld))
    nbytes = hip.bf16_image_bytes(b, c, ld)
    image = torch.full((nbytes,), 0x7f, dtype=torch.uint8, device=DEV)
    hip.bf16_image(xd, image, t, (g.to(DEV), be.to(DEV)), stats, EPS)
    torch.cuda.synchronize()
    assert guards_intact(whole), 'bf16_image wrote outside stats'
    out = stats.cpu()
    assert bool((out[:, :, t:] == 0).all())
    return out, image.cpu().view(BF16).view(b, (c + 15) // 16, 2, ld + 1, 8)


def layernorm(xd, t, g, be, out_dtype, absmax=False, in_place=False):
    """layernorm_channels into a guarded y (or onto a guarded copy of x): (y on the cpu, absmax on the cpu or None)."""
    b, c, ld = xd.shape
    whole, y = guarded((b, c, ld), out_dtype)
    if in_place:
        y.copy_(xd)
    whole_a, amax = guarded((b,)) if absmax else (None, None)
    hip.layernorm_channels(y if in_place else xd, g.to(DEV), be.to(DEV), y, t, EPS, amax)
    torch.cuda.synchronize()
    assert guards_intact(whole), 'layernorm_channels wrote outside y'
    assert whole_a is None or guards_intact(whole_a), 'layernorm_channels wrote outside absmax'
    out = y.cpu()
    assert bool((out[:, :, t:] == 0).all()), 'pitch columns of y are not 0'
    return out, (amax.cpu() if absmax else None)


def fma32(a, b, c):
    """fp32 fused multiply-add of fp32 tensors: the product is exact in float64, the sum is rounded there and once more to fp32."""
    return (a.double() * b.double() + c.double()).float()


# ---- A. statistics against fp64 and the model (and the sibling half of B) -----------------------------------------------------------------
def statistics_of_every_producer(x, t, dtype, g, be):
    """The (mean, rstd) rows of every kernel that calls tile_statistics on this storage type, asserted bit-equal; the batch's rows."""
    xd = put(x, dtype)
    stats = channel_stats(xd, t)
    for u in range(BATCH):
        alone = channel_stats(put(x[u:u + 1], dtype), t)
        assert same_bits(alone[0], stats[u]), f'utterance {u} alone differs from the batch'
    others = {'bf16_image': bf16_image(xd, t, g, be)[0]}
    if dtype == F32:
        others['layernorm_split_image'] = split_image(xd, t, g, be)[0]
    for name, got in others.items():
        assert same_bits(got, stats), f'{name}: statistics differ from channel_stats'
    return stats


def the_model_form(xc, mean, rstd):
    """Which contracted form of the model the kernel IS, column by column: (the form, the share of columns with its bits)."""
    got = np.stack([mean, rstd])
    forms = [con for n in range(len(lm.CONTRACTIONS) + 1) for con in itertools.combinations(lm.CONTRACTIONS, n)]
    hits = [float((np.stack(lm.tile_statistics(xc, contract=con)) == got).all(axis=0).mean()) for con in forms]
    return forms[int(np.argmax(hits))], max(hits)


def measured(full, dtype, g, be):
    """Every frame count of this storage type as a prefix of ``full`` (BATCH, c, T_MAX), through every producer: (columns (c, N), mean (N,),
    rstd (N,)).  A column's statistics depend on that column alone, so the model and fp64 are evaluated once for all frame counts."""
    cols = []
    for t in FRAMES[dtype]:
        x = full[:, :, :t].contiguous()
        stats = statistics_of_every_producer(x, t, dtype, g, be)
        cols.append((lm.columns(x.numpy()), stats[:, 0, :t].reshape(-1).numpy(), stats[:, 1, :t].reshape(-1).numpy()))
    return tuple(np.concatenate([col[i] for col in cols], axis=-1) for i in range(3))


def assert_as_good_as_the_model(xc, mean, rstd, label, note=''):
    m_gpu, e_gpu = (float(e.max()) for e in lm.errors(mean, rstd, xc))
    m_model, e_model = (float(e.max()) for e in lm.errors(*lm.tile_statistics(xc), xc))
    print(f'{label} rstd e_gpu {e_gpu:.2e} e_model {e_model:.2e} ratio {e_gpu / max(e_model, 1e-30):5.2f} | mean e_gpu {m_gpu:.2e} e_model {m_model:.2e}{note}')
    if e_gpu > max(4.0 * e_model, 1e-6) or m_gpu > max(4.0 * m_model, 1e-6):   # before calling it a bug: what the contracted forms give
        for con in [(name,) for name in lm.CONTRACTIONS] + [lm.CONTRACTIONS]:
            errs = [float(e.max()) for e in lm.errors(*lm.tile_statistics(xc, contract=con), xc)]
            print(f'    model contracted at {con}: (mean, rstd) errors {errs}')
    assert e_gpu <= max(4.0 * e_model, 1e-6), (label, 'rstd', e_gpu, e_model)
    assert m_gpu <= max(4.0 * m_model, 1e-6), (label, 'mean', m_gpu, m_model)


@pytest.mark.parametrize('dtype,c', CASES, ids=IDS)
def test_statistics_vs_fp64_and_model(dtype, c):
    g, be = affine(c)
    for kind in lm.FAMILIES:
        xc, mean, rstd = measured(draw(kind, c, dtype), dtype, g, be)
        note = ''
        if kind == 'offset30':                                      # (information: which products are fused is the compiler's choice)
            form, share = the_model_form(xc, mean, rstd)
            note = f' | {100 * share:.1f}% of the columns are the bits of the model contracted at {form or "nothing"}'
        assert_as_good_as_the_model(xc, mean, rstd, f'c {c:5d} {kind:17s}', note)


# ---- B. layernorm_channels from those statistics ---------------------------------------------------------------------------------------
def restatements(x, stats, g, be, t, out_dtype):
    """((x - mean) rstd) g + b with the last two operations rounded separately, and as one fused multiply-add; rounded once to bf16
    for a bf16 result; pitch columns 0.  x (b, c, t) fp32 values, stats (b, 2, ld)."""
    b, c, _ = x.shape
    ld = stats.shape[2]
    n = (x - stats[:, 0:1, :t].expand_as(x)) * stats[:, 1:2, :t].expand_as(x)
    ge, bee = g[None, :, None].expand_as(x).contiguous(), be[None, :, None].expand_as(x).contiguous()
    out = []
    for v in (n * ge + bee, fma32(n, ge, bee)):
        y = torch.zeros(b, c, ld, dtype=out_dtype)
        y[:, :, :t] = v.to(out_dtype)
        out.append(y)
    return out


@pytest.mark.parametrize('dtype,c', CASES, ids=IDS)
def test_layernorm_channels_is_its_statistics_applied(dtype, c):
    g, be = affine(c)
    full = draw('benign', c, dtype)
    forms = set()
    for t in FRAMES[dtype]:
        x = full[:, :, :t].contiguous()
        xd = put(x, dtype)
        stats = channel_stats(xd, t)
        for out_dtype in ((F32,) if dtype == F32 else (BF16, F32)):
            y, _ = layernorm(xd, t, g, be, out_dtype)
            plain, fused = restatements(x, stats, g, be, t, out_dtype)
            is_plain, is_fused = bits(y) == bits(plain), bits(y) == bits(fused)
            assert bool((is_plain | is_fused).all()), (t, out_dtype, f'{int((~(is_plain | is_fused)).sum())} elements are neither restatement')
            forms.add((out_dtype, 'fused' if bool(is_fused.all()) else 'plain' if bool(is_plain.all()) else 'mixed'))
            if dtype == out_dtype:
                again, _ = layernorm(xd, t, g, be, out_dtype, in_place=True)
                assert same_bits(again, y), (t, 'in place differs from out of place')
            if dtype == F32:
                with_absmax, _ = layernorm(xd, t, g, be, F32, absmax=True)
                assert same_bits(with_absmax, y), (t, 'the absmax by-product changed y')
            for u in range(BATCH):
                alone, _ = layernorm(put(x[u:u + 1], dtype), t, g, be, out_dtype)
                assert same_bits(alone[0], y[u]), (t, out_dtype, f'utterance {u} alone differs from the batch')
    print(f'c {c}: y is {sorted(forms, key=str)}')
    assert all(form != 'mixed' for _, form in forms), forms        # one kernel, one compiler: the same form for every element


# ---- C. pitch columns of x and a dead chunk --------------------------------------------------------------------------------------------
def every_output(x, t, dtype, g, be, ld=None, pitch=0.0):
    """name -> live part of every output of every kernel on this storage type (images up to row t, statistics and y up to frame t)."""
    xd = put(x, dtype, ld, pitch)
    out = {'channel_stats': channel_stats(xd, t)[:, :, :t]}
    st, img = bf16_image(xd, t, g, be)
    assert bool((bits(img[:, :, :, t + 1:]) == 0).all()) and bool((bits(img[:, :, :, 0]) == 0).all()), 'bf16_image: pitch rows or row 0 not zero'
    out['bf16_image.stats'], out['bf16_image.image'] = st[:, :, :t], img[:, :, :, :t + 1]
    if dtype == F32:
        st, bound, img = split_image(xd, t, g, be)
        assert bool((bits(img[:, :, :, :, t + 1:]) == 0).all()) and bool((bits(img[:, :, :, :, 0]) == 0).all()), 'split image: pitch rows or row 0 not zero'
        out['split_image.stats'], out['split_image.bound'], out['split_image.image'] = st[:, :, :t], bound, img[:, :, :, :, :t + 1]
        y, amax = layernorm(xd, t, g, be, F32, absmax=True)
        out['layernorm+absmax.y'], out['layernorm+absmax.absmax'] = y[:, :, :t], amax
    for out_dtype in ((F32,) if dtype == F32 else (BF16, F32)):
        out[f'layernorm->{out_dtype}'] = layernorm(xd, t, g, be, out_dtype)[0][:, :, :t]
    return out


@pytest.mark.parametrize('dtype,c,t', [(F32, 17, 5), (F32, 113, 65), (F32, 3, 129), (BF16, 17, 9), (BF16, 113, 129), (BF16, 3, 257)],
                         ids=lambda v: 'bf16' if v == BF16 else 'f32' if v == F32 else str(v))
def test_pitch_columns_of_x_and_a_dead_chunk_change_nothing(dtype, c, t):
    g, be = affine(c)
    x = draw('benign', c, dtype)[:, :, :t].contiguous()
    ld, chunk = hip.row_pitch(t, dtype), 8 if dtype == BF16 else 4
    assert ld > t                                                   # there ARE pitch columns
    want = every_output(x, t, dtype, g, be)
    for ld_, pitch in ((ld, NAN), (ld + chunk, 0.0), (ld + chunk, NAN)):
        got = every_output(x, t, dtype, g, be, ld_, pitch)
        assert got.keys() == want.keys()
        for name in want:
            assert same_bits(got[name], want[name]), (name, ld_, pitch)


# ---- D. the absmax by-product ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', lm.CHANNEL_EDGES)
def test_absmax_is_the_largest_magnitude_of_y(c):
    g, be = affine(c)
    for kind, t in itertools.product(('benign', 'first16_outliers'), (3, 65, 257)):
        x = draw(kind, c, F32)[:, :, :t].contiguous()
        y, amax = layernorm(put(x, F32), t, g, be, F32, absmax=True)
        assert same_bits(amax, y[:, :, :t].abs().amax(dim=(1, 2))), (kind, t, amax)


def test_absmax_drops_non_finite_values():
    c, t = 49, 65
    g, be = affine(c)
    x = draw('benign', c, F32)[:, :, :t].contiguous()
    y, amax = layernorm(put(x, F32), t, g, be, F32, absmax=True)
    for bad in (INF, -INF, NAN):
        xb = x.clone()
        xb[1, 20, 7] = bad                                          # poisons frame 7 of utterance 1: its statistics are not finite
        yb, amaxb = layernorm(put(xb, F32), t, g, be, F32, absmax=True)
        assert same_bits(yb[0], y[0]) and same_bits(yb[2], y[2]) and same_bits(amaxb[[0, 2]], amax[[0, 2]]), bad
        keep = [f for f in range(t) if f != 7]
        assert same_bits(yb[1, :, keep], y[1, :, keep]), bad          # the other frames of utterance 1 are untouched as well
        live = yb[1, :, :t]
        assert bool(torch.isfinite(amaxb[1])), (bad, amaxb)
        assert float(amaxb[1]) == float(torch.where(torch.isfinite(live), live.abs(), torch.zeros_like(live)).max()), (bad, amaxb)
        assert float(amaxb[1]) >= float(y[1, :, keep].abs().max()) > 0
    # an utterance every frame of which is poisoned: nothing finite is left of it, its absmax is 0
    xb = x.clone()
    xb[1, 0, :] = INF
    yb, amaxb = layernorm(put(xb, F32), t, g, be, F32, absmax=True)
    assert not bool(torch.isfinite(yb[1, :, :t]).any())
    assert float(amaxb[1]) == 0.0 and same_bits(amaxb[[0, 2]], amax[[0, 2]])


# ---- E. input_range ----------------------------------------------------------------------------------------------------------------------
def range_input(c, t, bad_value, seed):
    """(BATCH, c, t): utterance 0 ordinary (frames of very different loudness, some silent), 1 holds one non-finite sample (bad_value
    None: none), 2 is silent."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(BATCH, c, t, generator=gen) * torch.exp(torch.rand(BATCH, 1, t, generator=gen) * 10.0 - 8.0)
    if t > 5:
        x[:, :, ::5] = 0.0                                           # silent frames: not the quietest NON-silent frame
    x[2] = 0.0
    if bad_value is not None:
        x[1, c // 2, (2 * t) // 3] = bad_value
    return x


def range_expected(x):
    a = x.abs()
    finite = torch.isfinite(x)
    a = torch.where(finite, a, torch.zeros_like(a))
    per_frame = a.amax(dim=1)                                        # (b, t): the frame's largest finite magnitude
    quiet = torch.where(per_frame > 0, per_frame, torch.full_like(per_frame, INF)).amin(dim=1)
    return a.amax(dim=(1, 2)), quiet, (~finite).any(dim=2).any(dim=1)


def input_range(x, ld, pitch=0.0):
    b, c, t = x.shape
    xd = torch.full((b, c, ld), pitch, device=DEV)
    xd[:, :, :t] = x.to(DEV)
    whole, out = guarded((b, 4))
    hip.input_range(xd, t, out)
    torch.cuda.synchronize()
    assert guards_intact(whole), 'input_range wrote outside range'
    return out.cpu()


@pytest.mark.parametrize('c', [1, 3, 4, 5, 80])
def test_input_range_is_exact(c):
    for t, bad in itertools.product((1, 3, 255, 256, 257, 1027), (None, NAN, INF, -INF)):
        x = range_input(c, t, bad, seed=c * 10000 + t)
        hi, quiet, flag = range_expected(x)
        assert float(hi[2]) == 0.0 and float(quiet[2]) == INF and flag.tolist() == [False, bad is not None, False]
        assert t < 255 or float(quiet[0]) < float(hi[0]) * 2.0 ** -4                    # the two figures of utterance 0 are different frames'
        routes = [(hip.round_up4(t), 0.0), (hip.round_up4(t) + 4, 0.0), (hip.round_up4(t) + 4, NAN)]      # 16-byte loads; a dead chunk; NaN in it
        if hip.round_up4(t) > t:
            routes.append((hip.round_up4(t), NAN))
        if t % 2:
            routes.append((t, 0.0))                                  # ld odd: the scalar route
        for ld, pitch in routes:
            got = input_range(x, ld, pitch)
            what = (t, bad, ld, pitch, got)
            assert same_bits(got[:, 0], hi), what
            assert same_bits(got[:, 1], quiet), what
            assert ((got[:, 2] != 0) == flag).all(), what
            assert got[2].tolist()[:3] == [0.0, INF, 0.0], what
