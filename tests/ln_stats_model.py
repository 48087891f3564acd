"""tile_statistics (nb_asr_amd/csrc/layernorm.hip) restated in numpy fp32, every operation rounded on its own; no GPU.

The documented order, for one frame column of C channels:

    16 row slots; slot r folds the channels r, r + 16, ... in ascending order:
        shift = the slot's first channel;  d = x - shift;  s1 += d;  s2 = fma(d, d, s2)
        dm = s1 / n;  slot mean = shift + dm;  M2 = max(s2 - dm s1, 0)
    Chan's merge over the slots 0 .. 15 from (0, 0, 0), slots without a channel left out:
        tot = n + nb;  d = mean_b - mean;  mean += d (nb / tot);  M2 += M2_b + d d (n nb / tot);  n = tot
    rstd = 1 / sqrt(M2 / n + eps)

The (8, 4, 1)-rows-in-flight loops of the kernel only change when a channel is LOADED, never when it is folded, so they do not appear
here: a kernel that gets one of their bounds wrong folds a channel twice or not at all and leaves this model by far more than rounding.

``contract`` names the expressions that a compiler may evaluate with ONE rounding (a fused multiply-add) instead of two:

    'm2'     s2 - dm s1              as fma(-dm, s1, s2)
    'mean'   mean + d (nb / tot)     as fma(d, nb / tot, mean)
    'merge'  M2_b + (d d) X          as fma(d d, X, M2_b),   X = n nb / tot

For bf16 storage the inputs are bf16-valued fp32 numbers; nothing else changes.  Everything is vectorised over the frame columns:
x is (C, N) for N independent columns (``columns`` turns a (batch, C, frames) tensor into that).
"""
import numpy as np

F32 = np.float32
ROWS = 16                      # LN_ROWS
CONTRACTIONS = ('m2', 'mean', 'merge')


def fma32(a, b, c):
    """fp32 fused multiply-add of fp32 arrays: the product is exact in float64, the sum is rounded there and once more to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def columns(x):
    """(batch, C, frames) -> (C, batch * frames), column b * frames + t = frame t of utterance b."""
    x = np.asarray(x, dtype=F32)
    b, c, t = x.shape
    return np.ascontiguousarray(x.transpose(1, 0, 2).reshape(c, b * t))


def slot_partials(x, contract=()):
    """The 16 row partials of x (C, N): counts (16,) and means, M2 (16, N); a slot without a channel has count 0."""
    x = np.ascontiguousarray(x, dtype=F32)
    c, n_col = x.shape
    live = min(ROWS, c)
    shift = np.zeros((ROWS, n_col), F32)
    shift[:live] = x[:live]
    s1 = np.zeros((ROWS, n_col), F32)
    s2 = np.zeros((ROWS, n_col), F32)
    for c0 in range(0, c, ROWS):                                   # step k of every slot at once: channels c0 .. c0 + 15
        m = min(ROWS, c - c0)
        d = x[c0:c0 + m] - shift[:m]
        s1[:m] = s1[:m] + d
        s2[:m] = fma32(d, d, s2[:m])
    cnt = np.array([len(range(r, c, ROWS)) for r in range(ROWS)], F32)
    fn = np.maximum(cnt, F32(1))[:, None]
    dm = s1 / fn
    mean = shift + dm
    if 'm2' in contract:
        m2 = np.maximum(fma32(-dm, s1, s2), F32(0))
    else:
        m2 = np.maximum(s2 - dm * s1, F32(0))
    return cnt, mean, m2


def chan_merge(n, mean, m2, nb, mean_b, m2_b, contract=()):
    """One merge; n, nb fp32 scalars, the rest (N,) fp32 arrays."""
    tot = F32(n + nb)
    d = mean_b - mean
    r = F32(nb / tot)
    mean = fma32(d, np.full_like(d, r), mean) if 'mean' in contract else mean + d * r
    xk = F32(F32(n * nb) / tot)
    dd = d * d
    m2 = m2 + (fma32(dd, np.full_like(d, xk), m2_b) if 'merge' in contract else m2_b + dd * xk)
    return tot, mean, m2


def tile_statistics(x, eps=1e-3, contract=(), minmax=False):
    """x (C, N) fp32 -> (mean, rstd) of every column, each (N,) fp32; with ``minmax`` also the extrema (lo, hi) over the channels."""
    assert set(contract) <= set(CONTRACTIONS), contract
    x = np.ascontiguousarray(x, dtype=F32)
    cnt, means, m2s = slot_partials(x, contract)
    n_col = x.shape[1]
    n, mean, m2 = F32(0), np.zeros(n_col, F32), np.zeros(n_col, F32)
    for k in range(ROWS):
        if cnt[k] > 0:
            n, mean, m2 = chan_merge(n, mean, m2, cnt[k], means[k], m2s[k], contract)
    rstd = F32(1) / np.sqrt(m2 / max(n, F32(1)) + F32(eps))
    assert mean.dtype == F32 and rstd.dtype == F32
    if minmax:
        return mean, rstd, x.min(axis=0), x.max(axis=0)
    return mean, rstd


def truth(x, eps=1e-3):
    """fp64 statistics of the fp32 values x (C, N): mean, rstd, sd, and the conditioning |mean| sd / (var + eps) of every column."""
    x = np.asarray(x, dtype=np.float64)
    mean, var = x.mean(axis=0), x.var(axis=0)
    sd = np.sqrt(var)
    return mean, 1.0 / np.sqrt(var + eps), sd, np.abs(mean) * sd / (var + eps)


def errors(mean, rstd, x, eps=1e-3):
    """Per column: the error of ``mean`` in units of max(sd, sqrt(eps)) and the relative error of ``rstd``, against fp64."""
    mean64, rstd64, sd, _ = truth(x, eps)
    return np.abs(mean - mean64) / np.maximum(sd, np.sqrt(eps)), np.abs(rstd - rstd64) / rstd64


# ---- the input families of the edge tests -------------------------------------------------------------------------------------------
FAMILIES = ('benign', 'offset30', 'offset1000', 'relu_sparse', 'first16_outliers', 'constant', 'mixed_scale')
WELL_CONDITIONED = ('benign', 'mixed_scale', 'constant')
CONDITIONED = ('offset30', 'offset1000', 'relu_sparse', 'first16_outliers')
CHANNEL_EDGES = (1, 3, 15, 16, 17, 48, 49, 64, 65, 112, 113, 127, 128, 129, 176, 177, 240, 241, 600, 1200)


def family(kind, shape, seed):
    """One draw (batch, C, frames) fp32 of an input family, a fixed function of (kind, shape, seed)."""
    b, c, t = shape
    rng = np.random.default_rng([FAMILIES.index(kind), b, c, t, seed])
    z = rng.standard_normal(shape)
    first = min(ROWS, c)
    if kind == 'benign':
        x = 0.7 + 2.0 * z
    elif kind == 'offset30':
        x = 30.0 + z
    elif kind == 'offset1000':
        x = 1000.0 + z
    elif kind == 'relu_sparse':
        x = np.maximum(z - 1.5, 0.0)
        hot = rng.integers(0, first, (b, t))
        np.put_along_axis(x, hot[:, None, :], 20.0, axis=1)
    elif kind == 'first16_outliers':
        x = 0.1 * z
        x[:, :first] += 20.0 * np.where(rng.standard_normal((b, first, t)) < 0, -1.0, 1.0)
    elif kind == 'constant':
        x = np.full(shape, 3.25)
    elif kind == 'mixed_scale':
        x = z * np.exp(rng.uniform(-12.0, 3.0, (b, 1, t)))
    else:
        raise ValueError(kind)
    return x.astype(F32)


BOUND_A, BOUND_B, BOUND_C = 4.0, 3.0, 1.0


def conditioned_bound(c, cond):
    """The stated bound of the relative error of rstd for the conditioned families, per frame column (see test_ln_stats_host.py):
    2^-24 (A + B ceil(C / 16) + C' cond), cond = |mean| sd / (var + eps)."""
    return 2.0 ** -24 * (BOUND_A + BOUND_B * -(-c // ROWS) + BOUND_C * cond)
