"""The geometry of streaming inference (nb_asr_amd/streaming.py), on the CPU: the lookahead the planner derives is the one a float64
perturbation of the oracle shows, and driving the oracle's per-layer functions through the planner's windows -- chunk by chunk, LSTM
state carried -- reproduces the oracle's whole-utterance forward to float64 round-off with exactly nbasr_output_frames(T) frames."""
import pytest
import torch
import torch.nn.functional as F

import cases
import nb_asr_amd as nb
from nb_asr_amd import hip, streaming
from nb_asr_amd.weights import keyed_fill_, keyed_input
from oracle import asr_oracle as oracle

ARCH_LZ = [[0, 1], [5, 0, 1], [1, 1, 0, 1]]          # a `linear` main op, a `zero` main op with a skip, a conv on the zero node


def params_of(arch, use_rnn, seed=1235):
    m = nb.get_model(arch, use_rnn=use_rnn, dropout_rate=0.0)
    keyed_fill_(m, seed=seed, mode='lively')
    return {k: v.detach().double() for k, v in m.state_dict().items()}


def test_pad_rule_is_the_library_rule():
    for k, d in ((5, 1), (5, 2), (7, 1), (7, 2), (8, 1)):
        for s in (1, 2):
            assert streaming.pad_amounts(k, d, s) == hip.pad_amounts(k, d, s)


def test_cell_context_follows_every_path():
    assert streaming.cell_context(cases.ARCH_A) == (0, 12)
    assert streaming.cell_context(cases.ARCH_D) == (14, 12)
    assert streaming.cell_context(cases.ARCH_M) == (4, 4)
    assert streaming.cell_context(ARCH_LZ) == (0, 4)
    assert streaming.cell_context([[5, 0], [5, 0, 0], [5, 0, 0, 0]]) == (0, 0)        # all zero: the cell reads nothing
    assert streaming.cell_context([[4, 0], [0, 1, 0], [5, 0, 1, 0]]) == (8, 4)         # the conv reaches the output through skips


@pytest.mark.parametrize('name,arch,pos', [('A', cases.ARCH_A, 700), ('D', cases.ARCH_D, 700), ('M', cases.ARCH_M, 700), ('LZ', ARCH_LZ, 600)])
def test_lookahead_matches_a_perturbation_of_the_oracle(name, arch, pos):
    """Perturb input frame ``pos`` of a float64 oracle forward (use_rnn=False): the first logit frame that changes is the first whose
    lookahead reaches ``pos`` (4 o + lookahead >= pos), and the last one the last whose left context does.

    The perturbation is a NaN: it travels along every path of the receptive field whatever the weights (0 x NaN is NaN; ReLU and the
    clamp keep it), so the measured field is the structural one.  A finite perturbation measures less wherever the longest path's
    contribution -- one tap of every convolution on it, ~50 of them -- falls below float64 resolution of the frame's value: ARCH_A (no
    skips: the longest path is the only one) shows its full 506 frames that way too, the skip architectures D and M only 232 / 148."""
    t = 1200
    specs = streaming.stage_specs(arch, use_rnn=False)
    la = streaming.lookahead_frames(specs)
    p = params_of(arch, False)
    x = keyed_input(1, t, seed=2).double()
    x[:, :, pos] = float('nan')
    y = oracle.asr_forward(p, arch, x, use_rnn=False, dtype=torch.float64)
    changed = torch.isnan(y).any(dim=2).any(dim=0).nonzero().flatten()
    first, last = int(changed[0]), int(changed[-1])
    left = sum(sp.left * sp.rate for sp in specs)
    print(f'{name}: lookahead {la} frames, left context {left}; NaN outputs {first}..{last}')
    assert first == max(0, -(-(pos - la) // 4))
    assert last == min((pos + left) // 4, t // 4 - 1)
    if name == 'A':                                      # the finite perturbation agrees where no skip path drowns the long one
        x[:, :, pos] = 0.0
        y0 = oracle.asr_forward(p, arch, x, use_rnn=False, dtype=torch.float64)
        x[:, :, pos] = 1.0
        y1 = oracle.asr_forward(p, arch, x, use_rnn=False, dtype=torch.float64)
        assert int(((y1 - y0).abs().amax(dim=(0, 2)) > 0).nonzero()[0]) == first


def replay(arch, use_rnn, x, sizes, p):
    """The oracle's per-layer float64 functions driven through the planner: every stage keeps its window as a tensor, rebuilt from its
    retained frames and the producer's kept frames exactly as the session's windows are."""
    names = oracle.arch_names(arch)
    specs = streaming.stage_specs(arch, use_rnn)
    planner = streaming.StreamPlanner(specs)
    b = x.shape[0]
    windows = [x.new_zeros(b, sp.c_in, 0) for sp in specs]
    hc = None
    outs, at = [], 0
    steps = [(n, False) for n in sizes] + [(0, True)]
    for n, final in steps:
        plans = planner.step(n, final)
        new = x[:, :, at:at + n]
        at += n
        logits = x.new_zeros(b, 0, 49)
        for k, (sp, plan) in enumerate(zip(specs, plans)):
            if plan is None:
                new = None
                continue
            old = windows[k]
            win = torch.cat([old[:, :, plan.hist_off:plan.hist_off + plan.n_hist], new[:, :, :plan.n_new]], 2) if plan.n_new else \
                old[:, :, plan.hist_off:plan.hist_off + plan.n_hist]
            assert win.shape[2] == plan.b - plan.a
            windows[k] = win
            if not plan.compute:
                new = None
                continue
            k0, k1 = plan.c - plan.a // sp.stride, plan.d - plan.a // sp.stride
            pre = f'model.{sp.layer}.'
            if sp.kind == 'dense':
                y = oracle.pad_conv_relu(win, p[pre + 'conv.weight'], p[pre + 'conv.bias'], 1, sp.stride, 1)
                y = oracle.layer_norm_channels(y, p[f'model.{sp.layer + 1}.weight'], p[f'model.{sp.layer + 1}.bias'])
            elif sp.kind == 'cell':
                y = oracle.cell_forward(win, names, p, pre)
            elif sp.kind == 'lstm':
                lstm = torch.nn.LSTM(sp.c_in, sp.c_out, batch_first=True).double()
                with torch.no_grad():
                    for w in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0'):
                        getattr(lstm, w).copy_(p[pre + w])
                    h, hc = lstm(win.permute(0, 2, 1), hc)
                y = h.permute(0, 2, 1)
            else:
                y = F.linear(win.permute(0, 2, 1), p[pre + 'weight'], p[pre + 'bias']).permute(0, 2, 1)
            new = y[:, :, k0:k1]
            if sp.kind == 'head':
                logits = new.permute(0, 2, 1)
        outs.append(logits)
    return outs, planner


def ragged(t):
    sizes, pattern, i = [], (3, 0, 41, 200, 1, 17, 96, 5, 160), 0
    while sum(sizes) < t:
        sizes.append(min(pattern[i % len(pattern)], t - sum(sizes)))
        i += 1
    return sizes


@pytest.mark.parametrize('arch,use_rnn,t,kind', [
    (cases.ARCH_D, True, 300, 1), (cases.ARCH_M, True, 650, 7), (cases.ARCH_A, True, 900, 160), (cases.ARCH_D, True, 900, 'ragged'),
    (cases.ARCH_M, False, 333, 'whole'), (ARCH_LZ, True, 700, 'ragged'), (cases.ARCH_D, False, 700, 160),
])
def test_planner_replay_reproduces_the_whole_forward(arch, use_rnn, t, kind):
    p = params_of(arch, use_rnn)
    x = keyed_input(2, t, seed=1).double()
    sizes = [t] if kind == 'whole' else ragged(t) if kind == 'ragged' else [min(kind, t - i) for i in range(0, t, kind)]
    outs, planner = replay(arch, use_rnn, x, sizes, p)
    got = torch.cat(outs, 1)
    want = oracle.asr_forward(p, arch, x, use_rnn=use_rnn, dtype=torch.float64)
    assert got.shape[1] == hip.output_frames(t) == want.shape[1]
    err = float((got - want).abs().max())
    assert err <= 1e-9 * float(want.abs().max()), err
    # windows stay within the bounds the session allocates for max_chunk = 160 (all chunks here are at most 200: 200 as the bound)
    caps = planner.capacities(200)
    assert all(h >= 0 for h in planner.have) and len(caps) == len(planner.specs)


def test_frames_are_emitted_as_soon_as_they_are_final():
    """After n input frames exactly the logit frames o with 4 o + lookahead < n exist; flush releases the rest."""
    specs = streaming.stage_specs(cases.ARCH_D, True)
    la = streaming.lookahead_frames(specs)
    planner = streaming.StreamPlanner(specs)
    total, have = 0, 0
    for n in [1] * 40 + [37, 0, 160, 3, 500, 160, 160, 2]:
        plans = planner.step(n)
        have += n
        if plans[-1] is not None:
            total += plans[-1].d - plans[-1].c
        assert total == max(0, -(-(have - la) // 4)), (have, total)
    plans = planner.step(0, final=True)
    total += plans[-1].d - plans[-1].c
    assert total == hip.output_frames(have)
    with pytest.raises(ValueError):
        planner.step(1)


def test_window_capacity_bound_holds():
    """The largest window every stage sees over many push patterns stays within the planner's bound for that max_chunk."""
    for arch in (cases.ARCH_A, cases.ARCH_D, cases.ARCH_M, ARCH_LZ):
        specs = streaming.stage_specs(arch, True)
        for max_chunk in (1, 7, 40, 160):
            planner = streaming.StreamPlanner(specs)
            caps = planner.capacities(max_chunk)
            for n in [max_chunk] * 30 + [1, max_chunk, 0, max_chunk // 2 + 1] * 10:
                for plans in (planner.step(n),):
                    for k, plan in enumerate(plans):
                        if plan is not None:
                            assert plan.b - plan.a <= caps[k], (arch, max_chunk, k)
            for k, plan in enumerate(planner.step(0, final=True)):
                if plan is not None:
                    assert plan.b - plan.a <= caps[k], (arch, max_chunk, k, 'flush')
