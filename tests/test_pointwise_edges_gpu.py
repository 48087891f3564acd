"""Edges of the per-frame GEMM's main loop and time-major epilogue (gemm_pointwise.hip), of the LayerNorm image pass
(normalize_split_kernel, layernorm.hip) and of the statistics merge (stats_finalize_kernel, grouped_conv.hip; described at its test),
at the smallest shapes that reach them.

The GEMM (tile = 128 rows x 256 frames, K-step = 32 channels, a ring of three step buffers fetched two steps ahead):

    c_in    32, 40, 96, 136      n_ks = 1 (nothing to fetch ahead), 2 (the second step is fetched in the prologue, none in the loop),
                                 3 (the ring is full, one fetch in the loop), 5 (the ring wraps)
    c_out   48, 130, 200         an inactive wave row; a second row tile with a 2-row remainder; the 4-row store at the c_out edge
                                 (the projection's c_out is 4 x hidden with hidden % 4 == 0, so it takes 48, 144, 208 instead: an inactive
                                 wave row; a second row tile whose lower wave row alone is active; a 16-row remainder in the upper one)
    frames  3, 67, 256, 257      one partial column block; a partial second wave column; a full tile; a second frame tile with one frame
    batch   1 and 3              every utterance of the batch of 3 is also run alone

both operand schemes, the time-major projection and the `linear` node with one LayerNorm-carrying skip.  Every case is checked
three ways: against an fp64 evaluation under the rule of tests/cases.py (assert_parity: `want` is the fp32 evaluation on the CPU, for
bf16 storage rounded once as the kernel rounds); bit-equal for an utterance alone and inside the batch; bit-equal when c_in is padded
by one more K-step of zero channels and zero weights.

The image pass: every byte of the image (zero rows, pitch rows, padded channels), the statistics and the bound against an fp32
restatement of the documented arithmetic -- statistics: the unchanged sibling kernel nbasr_channel_stats (same tile_statistics);
bound: (max_t max(hi - mean, mean - lo) rstd) max|gamma| + max|beta| as ONE fused multiply-add, times 1.0001f; image:
fmaf((x - mean) rstd, gamma, beta) 2^k, hi = fp16(v), lo = fp16(v - hi).
"""
import itertools
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
F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-3
FRAMES = (3, 67, 256, 257)
BATCH = 3


def rows(v, dtype):
    """(b, c, t) cpu tensor -> device tensor of the storage type at the row pitch, pitch columns zero."""
    b, c, t = v.shape
    out = torch.zeros(b, c, hip.row_pitch(t, dtype), dtype=dtype, device=DEV)
    out[:, :, :t] = v.to(dtype).to(DEV)
    return out


def gemm(scheme, swap, x, w, bias, bias2, skip, gamma, beta):
    """One launch on cpu operands (b, c_in, t), (c_out, c_in): the projection's gates (t, b, c_out) or the linear node's y (b, c_out, t),
    as float32 on the cpu; also the (mean, rstd) rows of the skip that the launch used (None for the projection)."""
    dtype = BF16 if scheme == 'bf16' else F32
    b, c_in, t = x.shape
    c_out = w.shape[0]
    xp = rows(x, dtype)
    ld = xp.shape[2]
    if scheme == 'bf16':
        packed, ws = hip.pack_pointwise_weights_bf16(w.to(DEV)), hip.pointwise_bf16_workspace(b, c_in, ld, DEV)
    else:
        packed, ws = hip.pack_pointwise_weights(w.to(DEV)), hip.pointwise_workspace(b, c_in, ld, DEV)
    if swap:
        y = torch.full((t, b, c_out), 7.0, device=DEV)
        fn = hip.lstm_input_projection_bf16 if scheme == 'bf16' else hip.lstm_input_projection_packed
        fn(xp, t, packed, bias.to(DEV), bias2.to(DEV), y, c_out // 4, ws, ln=None)
        torch.cuda.synchronize()
        return y.cpu(), None
    sp = rows(skip, dtype)
    stats = torch.zeros(b, 2, ld, device=DEV)
    hip.channel_stats(sp, stats, t, EPS)
    y = torch.full((b, c_out, ld), 7.0, dtype=dtype, device=DEV)
    fn = hip.linear_fused_bf16 if scheme == 'bf16' else hip.linear_fused_packed
    fn(xp, t, packed, c_out, bias.to(DEV), [sp], y, ws, ln=(stats, gamma.to(DEV), beta.to(DEV)), ln_on_x=False, ln_on_skip0=True)
    torch.cuda.synchronize()
    assert torch.all(y[:, :, t:] == 0)
    return y[:, :, :t].float().cpu(), stats[:, :, :t].cpu()


def evaluate(swap, x, w, bias, bias2, skip, gamma, beta, stats, dt):
    """The same map in precision `dt` on the cpu; the skip's LayerNorm from the statistics the launch used."""
    pre = torch.einsum('oc,bct->bot', w.to(dt), x.to(dt)) + bias.to(dt)[None, :, None]
    if swap:
        return (pre + bias2.to(dt)[None, :, None]).permute(2, 0, 1).contiguous()
    normed = (skip.to(dt) - stats[:, 0:1].to(dt)) * stats[:, 1:2].to(dt) * gamma.to(dt)[None, :, None] + beta.to(dt)[None, :, None]
    return pre.clamp(min=0.0, max=20.0) + normed


GEMM_CASES = [(scheme, swap, c_in, c_out) for scheme in ('f16', 'bf16') for swap in (True, False)
              for c_in in (32, 40, 96, 136) for c_out in ((48, 144, 208) if swap else (48, 130, 200))]


@pytest.mark.parametrize('scheme,swap,c_in,c_out', GEMM_CASES)
def test_gemm_edges(scheme, swap, c_in, c_out):
    dtype = BF16 if scheme == 'bf16' else F32
    for t in FRAMES:
        tag = f'pointwise_edges/{scheme}/{int(swap)}/{c_in}/{c_out}/{t}'
        p = cases.keyed_params({'weight': (c_out, c_in), 'bias': (c_out,), 'bias2': (c_out,), 'norm.weight': (c_out,), 'norm.bias': (c_out,)}, tag)
        p = {k: v.to(dtype).float() for k, v in p.items()}                       # bf16 scheme: the fp32 VALUES of bf16 parameters
        x = cases.keyed_x(tag, (BATCH, c_in, t)).to(dtype).float()
        x[:, :, t // 2:] *= 0.125                                                # the tile's scale is set by a few frames, exactly
        skip = cases.keyed_x(tag + '/skip', (BATCH, c_out, t)).to(dtype).float()
        args = (p['weight'], p['bias'], p['bias2'])
        ln = (p['norm.weight'], p['norm.bias'])
        got, stats = gemm(scheme, swap, x, *args, skip, *ln)
        what = f'{tag}'

        # 1. against fp64, under the rule of tests/cases.py
        want = evaluate(swap, x, *args, skip, *ln, stats, torch.float32)
        if dtype == BF16 and not swap:
            want = want.to(BF16).float()                                         # the ONE rounding of a bf16 result
        truth = evaluate(swap, x, *args, skip, *ln, stats, torch.float64)
        ratio, noise = cases.assert_parity(got, want, truth, what)
        print(f'{what}: err/tol vs fp32 {ratio:.3f}, fp32 vs fp64 {noise:.3f}')

        # 2. an utterance alone == the same utterance inside the batch
        for u in (0, BATCH - 1):
            alone, _ = gemm(scheme, swap, x[u:u + 1], *args, skip[u:u + 1], *ln)
            inside = got[:, u:u + 1] if swap else got[u:u + 1]
            assert torch.equal(alone, inside), f'{what}: utterance {u} alone differs from the batch'

        # 3. one more K-step of zero channels and zero weights changes no bit
        xz = torch.cat([x, torch.zeros(BATCH, 32, t)], dim=1)
        wz = torch.cat([p['weight'], torch.zeros(c_out, 32)], dim=1)
        padded, _ = gemm(scheme, swap, xz, wz, p['bias'], p['bias2'], skip, *ln)
        assert torch.equal(padded, got), f'{what}: zero-padding c_in by one K-step changed the result'


# ---- nbasr_layernorm_split_image ----------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fp32 fused multiply-add of fp32 tensors: the product is exact in float64, the sum is rounded there and once more to fp32."""
    return (a.double() * b.double() + c.double()).float()


def pow2_scale(bound):
    """2^k that brings the bound into [2^14, 2^15) (normalize_split_kernel)."""
    bits = bound.view(torch.int32)
    e = (bits >> 23) & 0xff
    k = torch.where((bits & 0x7fffffff) != 0, (127 + 14) - e, torch.zeros_like(e)).clamp(-126, 126)
    return ((127 + k) << 23).to(torch.int32).view(torch.float32)


IMAGE_CASES = [(c, ld, b) for c, ld, b in itertools.product((17, 40, 600), (4, 252, 260), (1, 9))] + [(17, 260, 64)]   # 64 x 2 tiles: grid z = 4
IMAGE_CASES += [(c, 260, 1) for c in (1, 16, 113, 129, 241)]                     # the channel loop of tile_statistics: empty row slots, 4 and 8 rows in flight, tails


@pytest.mark.parametrize('c,ld,b', IMAGE_CASES)
def test_layernorm_split_image_bits(c, ld, b):
    t = ld - 1 if ld == 4 else ld - 3                                            # frames < ld
    tag = f'pointwise_edges/image/{c}/{ld}/{b}'
    x = torch.zeros(b, c, ld)
    x[:, :, :t] = cases.keyed_x(tag, (b, c, t)) * 2.0 + 0.7
    x[0] *= 1e-3
    p = cases.keyed_params({'norm.weight': (c,), 'norm.bias': (c,)}, tag)
    g, be = p['norm.weight'], p['norm.bias']
    xd = x.to(DEV)
    stats, bound = torch.full((b, 2, ld), 7.0, device=DEV), torch.full((b,), 7.0, device=DEV)
    image = hip.split_image(b, c, ld, DEV)
    image.fill_(0x7f)
    hip.layernorm_split_image(xd, g.to(DEV), be.to(DEV), stats, bound, image, t, EPS)
    want_stats = torch.full((b, 2, ld), 7.0, device=DEV)
    hip.channel_stats(xd, want_stats, t, EPS)
    torch.cuda.synchronize()
    stats, bound = stats.cpu(), bound.cpu()
    assert torch.equal(stats, want_stats.cpu()), 'statistics differ from nbasr_channel_stats'
    assert torch.all(stats[:, :, t:] == 0)

    mean, rstd = stats[:, 0], stats[:, 1]                                         # (b, ld)
    hi, lo = x.max(dim=1).values, x.min(dim=1).values
    dev = (torch.maximum(hi - mean, mean - lo) * rstd).abs()[:, :t].max(dim=1).values
    want_bound = fma32(dev, g.abs().max().expand(b), be.abs().max().expand(b)) * torch.tensor(1.0001, dtype=torch.float32)
    assert torch.equal(bound, want_bound), (bound, want_bound)

    scale = pow2_scale(bound)[:, None, None]
    v = fma32((x - mean[:, None, :]) * rstd[:, None, :], g[None, :, None].expand_as(x), be[None, :, None].expand_as(x)) * scale
    v = torch.where(rstd[:, None, :] != 0, v, torch.zeros_like(v))               # ln_apply: 0 where rstd is 0 (the pitch columns)
    n_groups = (c + 15) // 16
    vp = torch.zeros(b, n_groups * 16, ld)
    vp[:, :c] = v
    h = vp.to(torch.float16)
    l = (vp - h.float()).to(torch.float16)
    want = torch.zeros(b, n_groups, 2, 2, ld + 1, 8, dtype=torch.float16)         # [b][group][split][half][1 + ld rows][8 ch]
    for s, term in enumerate((h, l)):
        want[:, :, s, :, 1:, :] = term.view(b, n_groups, 2, 8, ld).permute(0, 1, 2, 4, 3)
    got = image.cpu()[:want.numel() * 2].view(torch.float16).view(want.shape)
    assert image.numel() == want.numel() * 2
    same = got.view(torch.int16) == want.view(torch.int16)
    assert bool(same.all()), f'{int((~same).sum())} of {same.numel()} image halves differ; first at {(~same).nonzero()[0].tolist()}'


# ---- nbasr_grouped_stats_finalize ----------------------------------------------------------------------------------------------------
# The documented order (grouped_conv.hip): 8 part lanes, lane p merges the partials p, p + 8, ... in ascending order from (0, 0, 0);
# then the 8 lane results are merged, lane 0's first, lanes without a partial left out; rstd = 1 / sqrt(M2 / n + eps); Chan's merge
#     tot = n + nb;  d = mean_b - mean;  mean += d (nb / tot);  M2 += M2_b + d d (n nb / tot);  n = tot
# with nb = channels of the partial.  The reference below is that merge in plain fp32 operations, one rounding each.  A compiler may fuse
# `mean + d * r` and `M2_b + (d d) * X` into one rounding, and which of them it fuses is its own business, so the partials are chosen
# such that both products are EXACT and fusing changes nothing: every d that the merge meets is zero or a power of two.
#   * all partials of one lane carry the same mean M_p (d = 0 after the lane's first partial, whose r is 1 and X is 0), their M2 are
#     random: the lane's M2 is a sum of rounded fp32 additions in the lane's order -- any other order or dealing of the partials moves it;
#   * M_p = (the running mean of lanes 0 .. p-1) +- 2^-e, e in 5..7, all values in [1, 2) where fp32 has ONE spacing, so the sum that
#     makes M_p and the difference that recovers d are exact (the generator asserts it); the lane merge is then order-sensitive in the
#     mean (d r is rounded into it, r = n_p / tot differs per lane) and in M2.
SF_LANES = 8


def f32(v, like):
    """The count v as a full fp32 tensor: every operation below is then an element-wise fp32 operation on tensors, not a tensor-by-scalar
    one that the host library may rewrite (a division by a scalar as a multiplication by its reciprocal)."""
    return torch.full_like(like, float(v), dtype=torch.float32)


def chan_merge(n, mean, m2, nb, mean_b, m2_b):
    """One merge in fp32, every operation rounded on its own; all arguments (b, ld) fp32 tensors."""
    tot = n + nb
    d = mean_b - mean
    mean = mean + d * (nb / tot)
    m2 = m2 + (m2_b + (d * d) * ((n * nb) / tot))
    return tot, mean, m2


def finalize_partials(tag, nbs, b, ld):
    """part (nparts, b, 2, ld) as described above, for partials of nbs[k] channels."""
    nparts = len(nbs)
    lane_n = [sum(nbs[p::SF_LANES]) for p in range(SF_LANES)]
    u = torch.from_numpy(cases.keyed_uniform(f'{tag}/u', 5, (SF_LANES, 2, b, ld), 0.0, 1.0).astype('float32'))
    lane_mean = [(1.4 + 0.2 * u[0, 0]).float()]
    n, mu = f32(lane_n[0], lane_mean[0]), lane_mean[0]
    for p in range(1, SF_LANES):
        if lane_n[p] == 0:
            lane_mean.append(None)
            continue
        d = torch.where(u[p, 0] < 0.5, -1.0, 1.0) * torch.pow(2.0, -(5 + (u[p, 1] * 3).floor().clamp(max=2)))
        m_p = mu + d
        assert torch.equal(m_p - mu, d) and bool(((m_p >= 1) & (m_p < 2)).all())
        lane_mean.append(m_p)
        nb = f32(lane_n[p], mu)
        tot = n + nb
        mu = mu + d * (nb / tot)                                                  # d is a power of two: exact product
        n = tot
    part = torch.empty(nparts, b, 2, ld)
    m2 = torch.from_numpy(cases.keyed_uniform(f'{tag}/m2', 6, (nparts, b, ld), 0.1, 2.0).astype('float32'))
    for k in range(nparts):
        part[k, :, 0] = lane_mean[k % SF_LANES]
        part[k, :, 1] = m2[k] * float(nbs[k])
    return part


def finalize_reference(part, nbs, frames, eps):
    nparts, b, _, ld = part.shape
    lanes = []
    for p in range(SF_LANES):
        n, mean, m2 = torch.zeros(b, ld), torch.zeros(b, ld), torch.zeros(b, ld)
        for k in range(p, nparts, SF_LANES):
            n, mean, m2 = chan_merge(n, mean, m2, f32(nbs[k], mean), part[k, :, 0].contiguous(), part[k, :, 1].contiguous())
        lanes.append((n, mean, m2))
    n, mean, m2 = lanes[0]
    for p in range(1, SF_LANES):
        if float(lanes[p][0].max()) > 0:
            n, mean, m2 = chan_merge(n, mean, m2, *lanes[p])
    out = torch.zeros(b, 2, ld)
    out[:, 0, :frames] = mean[:, :frames]
    # the square root by way of float64: correctly rounded to fp32 (53 >= 2 x 24 + 2 bits), which the host library's fp32 routine is not
    root = torch.sqrt((m2 / n + f32(eps, m2)).double()).float()
    out[:, 1, :frames] = (torch.ones(b, ld) / root)[:, :frames]
    return out


# (parts, groups, groups per part, channels per group): a lone partial of 3 groups; 25 with a last partial of 3 groups instead of 4 (the
# node kernels' quads); 75 pairs (a fused cell at groups_per_part = 2); 100 per-group partials (the fused cell at the benchmark's width)
FINALIZE_CASES = [(1, 3, 4, 6), (25, 99, 4, 8), (75, 150, 2, 4), (100, 100, 1, 12)]


@pytest.mark.parametrize('ld', [4, 132])
@pytest.mark.parametrize('parts,groups,gpp,cg', FINALIZE_CASES)
def test_stats_finalize_bits(parts, groups, gpp, cg, ld):
    b, frames = 2, ld - 1 if ld == 4 else ld - 3                                 # frames < ld; ld 132: a second block with one live quad
    nbs = [cg * min(gpp, groups - gpp * k) for k in range(parts)]
    assert len(nbs) == (groups + gpp - 1) // gpp == parts and sum(nbs) == groups * cg
    part = finalize_partials(f'pointwise_edges/finalize/{parts}/{ld}', nbs, b, ld)
    want = finalize_reference(part, nbs, frames, EPS)
    ws = hip.grouped_stats_workspace(b, ld, groups, DEV)
    assert ws.numel() >= part.numel()
    ws.fill_(3.0)
    ws[:part.numel()] = part.reshape(-1).to(DEV)
    out = torch.full((b, 2, ld), 7.0, device=DEV)
    hip.grouped_stats_finalize(ws, out, groups * cg, frames, groups, EPS, groups_per_part=gpp)
    torch.cuda.synchronize()
    got = out.cpu()
    same = got.view(torch.int32) == want.view(torch.int32)
    worst = float(((got - want).abs() / want.abs().clamp_min(1e-30)).max())
    print(f'finalize parts {parts} ld {ld}: {int((~same[:, 0]).sum())} means and {int((~same[:, 1]).sum())} rstd of {same[:, 0].numel()} each differ, '
          f'worst relative difference {worst:.3e}')
    assert bool(same.all())
