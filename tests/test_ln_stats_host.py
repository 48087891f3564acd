"""What the documented order of tile_statistics (layernorm.hip) can and cannot deliver, measured on its numpy fp32 restatement
(tests/ln_stats_model.py) against fp64.  No GPU: the kernels are held to this model by tests/test_layernorm_edges_gpu.py.

Seven input families at 64 frames and the channel counts at which the kernel's channel loop changes its path.  The restatement is
as good as an fp32 two-pass evaluation where |mean| is of the order of the standard deviation, and NOT where it is far above it
or where a slot's first channel (its shift) is an outlier:

* the merge of the 16 slot partials carries UNSHIFTED fp32 means, so d = mean_b - mean is known to 2^-24 |mean| only, and the
  relative error of rstd grows like 2^-24 |mean| sd / (var + eps)                  (offset30, offset1000; first16_outliers at C = 3);
* a slot that opens on an outlier sums d d of the size of that outlier's distance for every later channel, so its
  s2 - dm s1 cancels: the error grows with the channels per slot, ceil(C / 16)     (relu_sparse, first16_outliers).

The bound that the conditioned families are held to has that form,

    |rstd - rstd64| / rstd64  <=  2^-24 (A + B ceil(C / 16) + C' |mean| sd / (var + eps))        per frame column,

with (A, B, C') = (4, 3, 1), fixed here (ln_stats_model.BOUND_*): the restatement stays inside it everywhere and reaches more than
half of it in every family, so it is neither vacuous nor, with the fixed seeds, too tight.  It is an observation about this
arithmetic, not a theorem.
"""
import numpy as np
import pytest
import torch

import ln_stats_model as lm

FRAMES = 64
SEED = 0


def twopass32(x):
    """torch's fp32 two-pass statistics of x (C, N)."""
    xt = torch.from_numpy(x)
    rstd = 1.0 / torch.sqrt(xt.var(dim=0, unbiased=False) + 1e-3)
    return xt.mean(dim=0).numpy(), rstd.numpy()


@pytest.fixture(scope='module')
def table():
    """{(family, C): measurements}, computed once; printed as the table that DESIGN.md quotes."""
    out = {}
    print()
    print(f'{"family":17s} {"C":>5s}  {"mean/sd":>9s} {"(2-pass)":>9s}  {"rstd rel":>9s} {"(2-pass)":>9s}  {"max cond":>9s}  {"of bound":>8s}')
    for kind in lm.FAMILIES:
        for c in lm.CHANNEL_EDGES:
            x = lm.columns(lm.family(kind, (1, c, FRAMES), SEED))
            mean, rstd = lm.tile_statistics(x)
            e_mean, e_rstd = lm.errors(mean, rstd, x)
            e_mean2, e_rstd2 = lm.errors(*twopass32(x), x)
            cond = lm.truth(x)[3]
            of_bound = float((e_rstd / lm.conditioned_bound(c, cond)).max())
            out[kind, c] = dict(e_mean=float(e_mean.max()), e_mean2=float(e_mean2.max()), e_model=float(e_rstd.max()),
                                e_twopass=float(e_rstd2.max()), cond=float(cond.max()), of_bound=of_bound)
            print(f'{kind:17s} {c:5d}  {e_mean.max():9.2e} {e_mean2.max():9.2e}  {e_rstd.max():9.2e} {e_rstd2.max():9.2e}  {cond.max():9.1f}  {of_bound:8.3f}')
    return out


def test_the_model_is_exact_where_the_arithmetic_is():
    """constant: every d is 0, the mean is 3.25 and M2 is 0 exactly, rstd = 1 / sqrt(eps) to the rounding of eps and of the root;
    one channel: the mean is the sample.  Empty slots (C < 16) take no part: C = 3 equals the three samples merged by hand."""
    for c in lm.CHANNEL_EDGES:
        mean, rstd = lm.tile_statistics(lm.columns(lm.family('constant', (1, c, FRAMES), SEED)))
        assert np.all(mean == np.float32(3.25))
        assert np.all(rstd == np.float32(1) / np.sqrt(np.float32(1e-3)))
    x = lm.columns(lm.family('benign', (1, 1, FRAMES), SEED))
    assert np.array_equal(lm.tile_statistics(x)[0], x[0])
    x = lm.columns(lm.family('benign', (1, 3, FRAMES), SEED))
    n, mean, m2 = np.float32(0), np.zeros(FRAMES, np.float32), np.zeros(FRAMES, np.float32)
    for k in range(3):
        n, mean, m2 = lm.chan_merge(n, mean, m2, np.float32(1), x[k], np.zeros(FRAMES, np.float32))
    got = lm.tile_statistics(x, minmax=True)
    assert np.array_equal(got[0], mean)
    assert np.array_equal(got[1], np.float32(1) / np.sqrt(m2 / np.float32(3) + np.float32(1e-3)))
    assert np.array_equal(got[2], x.min(axis=0)) and np.array_equal(got[3], x.max(axis=0))


def test_the_mean_is_as_good_as_two_pass(table):
    """The error of the mean in units of max(sd, sqrt(eps)), next to the two-pass value (printed with the table).  At an offset of
    1000 both sit near 2e-4 of sd: fp32 represents 1000 to 6e-5 and no evaluation does better.  Within 4 x two-pass or 1e-6."""
    for (kind, c), m in table.items():
        assert m['e_mean'] <= max(4.0 * m['e_mean2'], 1e-6), (kind, c, m)


def test_well_conditioned_families_match_two_pass(table):
    """The project's criterion for a producer of statistics (statistics_errors, test_dense_tilings_gpu.py): e <= max(4 e_ref, 1e-6)."""
    for kind in lm.WELL_CONDITIONED:
        for c in lm.CHANNEL_EDGES:
            m = table[kind, c]
            assert m['e_model'] <= max(4.0 * m['e_twopass'], 1e-6), (kind, c, m)


def test_the_conditioned_bound_is_neither_vacuous_nor_too_tight(table):
    """Inside the stated bound in every column of every case; every family uses at least a tenth of it somewhere."""
    for kind in lm.CONDITIONED:
        used = [table[kind, c]['of_bound'] for c in lm.CHANNEL_EDGES]
        print(f'{kind}: the model reaches {min(used):.3f} ... {max(used):.3f} of the bound')
        assert max(used) <= 1.0, (kind, used)
        assert max(used) >= 0.1, (kind, used)


def test_the_merge_carries_unshifted_means(table):
    """The property that the header of layernorm.hip describes: at 1000 + N(0, 1) and 17 channels (sixteen slots of one or two
    samples: all of the error is the merge's) rstd is more than 20 x worse than two-pass.  Should this fail because someone merged
    the slots relative to a common shift: correct that header, DESIGN.md and the bound above."""
    m = table['offset1000', 17]
    assert m['e_model'] > 20.0 * m['e_twopass'], m
    assert m['e_model'] > 20.0 * 2.0 ** -24


def test_contracted_forms_stay_inside_the_same_criteria():
    """A compiler may fuse any of the three contractible expressions; whichever it does, the criteria above still hold."""
    for con in (('m2',), ('mean',), ('merge',), lm.CONTRACTIONS):
        for kind in lm.FAMILIES:
            for c in lm.CHANNEL_EDGES:
                x = lm.columns(lm.family(kind, (1, c, FRAMES), SEED))
                e = lm.errors(*lm.tile_statistics(x, contract=con), x)[1]
                if kind in lm.WELL_CONDITIONED:
                    assert e.max() <= max(4.0 * lm.errors(*twopass32(x), x)[1].max(), 1e-6), (con, kind, c)
                else:
                    assert (e <= lm.conditioned_bound(c, lm.truth(x)[3])).all(), (con, kind, c)
