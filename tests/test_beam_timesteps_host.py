"""Per-token time steps of the beam search, the part that needs no GPU: the plain-Python model of the kernel's search
(beam_timesteps_model.py) is anchored on the decode oracle, the properties of its time steps are checked (the GPU tests compare the
device against this model), and the new C entry points are bound with the header's signatures and refuse bad arguments on the host."""
import inspect

import numpy as np
import pytest

import beam_timesteps_model as model
from nb_asr_amd import ctc, hip
from nbasr_header import declarations
from oracle import decode_oracle as oracle

NAMES = ('nbasr_ctc_beam_timed_workspace_bytes', 'nbasr_ctc_beam_search_timed', 'nbasr_ctc_beam_stream_timed_state_bytes',
         'nbasr_ctc_beam_stream_timed_init', 'nbasr_ctc_beam_stream_timed_step', 'nbasr_ctc_beam_stream_timed_finish')


# ---- the model is the oracle's search ------------------------------------------------------------------------------------------

def _assert_is_oracle(key, lp, width, top_n):
    want = oracle.ctc_beam_search(lp, width, cutoff_top_n=top_n)
    got = model.beam_search(lp, width, cutoff_top_n=top_n)
    assert len(got) == len(want), key
    for r, ((tok, score), (g_tok, g_score, steps)) in enumerate(zip(want, got)):
        assert g_tok == tok, (key, r, g_tok, tok)
        assert abs(g_score - score) <= 1e-6 * max(1.0, abs(score)), (key, r, g_score, score)
        assert len(steps) == len(tok)


@pytest.mark.parametrize('shape', model.ORACLE_SHAPES)
def test_model_equals_the_oracle_at_the_decode_test_shapes(shape):
    for key, lp, width, top_n in model.utterances(shape):
        _assert_is_oracle(key, lp, width, top_n)


def test_model_equals_the_oracle_on_the_narrow_beam_sweep():
    for key, lp, width, top_n in model.narrow_utterances():
        _assert_is_oracle(key, lp, width, top_n)


def test_model_beams_do_not_hang_on_float32_ties():
    """The seeds the GPU comparison uses: accumulating the scores in float64 changes no beam, so a rank is not decided by the last bit of
    an exp or a log, and the device is expected to return the model's beams everywhere."""
    cases = [u for shape in model.TIMED_SHAPES for u in model.utterances(shape)] + model.narrow_utterances()
    for key, lp, width, top_n in cases:
        assert model.same_beams(model.beam_search(lp, width, cutoff_top_n=top_n),
                                model.beam_search(lp, width, cutoff_top_n=top_n, dtype=np.float64)), key


# ---- what the model's time steps are ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', model.TIMED_SHAPES)
def test_model_timestep_properties_at_the_shapes(shape):
    for key, lp, width, top_n in model.utterances(shape):
        model.check_timestep_properties(key, lp, width, top_n, model.beam_search(lp, width, cutoff_top_n=top_n))


def test_model_timestep_properties_on_the_narrow_beam_sweep_which_hits_the_hard_paths():
    stats = {}
    for key, lp, width, top_n in model.narrow_utterances():
        model.check_timestep_properties(key, lp, width, top_n, model.beam_search(lp, width, cutoff_top_n=top_n, stats=stats))
    # the GPU comparison on these cases is not vacuous: records move (rule 2), and prefixes come back under live extensions of their old
    # node (rule 3)
    assert stats['updates'] > 0 and stats['recreated_under_live'] > 0, stats


def test_model_time_steps_need_not_increase_along_a_beam():
    """an earlier token's node may be updated after a later token's node was created (as in ctcdecode)."""
    found = False
    for _, lp, width, top_n in model.narrow_utterances():
        for _, _, steps in model.beam_search(lp, width, cutoff_top_n=top_n):
            found |= any(a >= b for a, b in zip(steps, steps[1:]))
    assert found


def test_model_width_one_on_peaked_input_gives_the_first_frame_of_every_argmax_run():
    lp, path = model.peaked(3, 60)
    for i in range(3):
        tokens, starts = model.argmax_run_starts(path[i].tolist())
        (tok, _, steps), = model.beam_search(lp[i].numpy(), 1)
        assert tok == tokens and steps == starts and len(tokens) > 10


# ---- interface -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', NAMES)
def test_symbols_are_bound_with_the_header_signature(name):
    """Declared, and loaded with the binding's types; that those are the header's is test_abi.py's check of every symbol."""
    assert name in declarations() and getattr(hip.load_library(), name).argtypes == hip.SIGNATURES[name][1]


def _err(lib):
    return lib.nbasr_last_error()


def test_timed_search_refuses_bad_arguments_on_the_host():
    lib = hip.load_library()
    p = 16                                            # a non-NULL, 8-byte aligned stand-in: every case is refused before a launch
    #      log_probs, lengths, ws, beams, scores, timesteps, beam_lens, batch, frames, classes, width, blank, top_n
    ok = [p, None, p, p, p, p, p, 2, 5, 49, 12, 0, 40]

    def search(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[{'ws': 2, 'timesteps': 5, 'lens': 6, 'classes': 9, 'width': 10}[k]] = v
        return lib.nbasr_ctc_beam_search_timed(*a, None)
    assert search(timesteps=None) == -3 and b'nbasr_ctc_beam_search_timed: NULL pointer' in _err(lib)
    assert search(ws=None) == -3 and search(lens=None) == -3
    assert search(width=33) == -1 and b'beam_width=33' in _err(lib)
    assert search(classes=65) == -1 and b'classes=65' in _err(lib)
    assert search(ws=20) == -2 and b'8-byte aligned' in _err(lib)
    # the timed pool is twice the untimed one (a node is two int2), the pruned copy of the log-probabilities is the same
    assert lib.nbasr_ctc_beam_timed_workspace_bytes(2, 10, 49, 12) == 2 * (10 * 12 + 1) * 16 + 2 * 10 * 49 * 4
    assert lib.nbasr_ctc_beam_workspace_bytes(2, 10, 49, 12) == 2 * (10 * 12 + 1) * 8 + 2 * 10 * 49 * 4
    assert lib.nbasr_ctc_beam_timed_workspace_bytes(0, 10, 49, 12) == 0


def test_timed_stream_refuses_bad_arguments_on_the_host():
    lib = hip.load_library()
    p = 16
    #      log_probs, lengths, state, ws, committed, c_frames, c_counts, partial, p_frames, p_counts, usage, batch, frames, classes, width, blank, top_n, pool
    ok = [p, None, p, p, p, p, p, p, p, p, p, 2, 5, 49, 12, 0, 40, 100]

    def step(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[{'state': 2, 'c_frames': 5, 'p_frames': 8, 'usage': 10, 'width': 14, 'pool': 17}[k]] = v
        return lib.nbasr_ctc_beam_stream_timed_step(*a, None)
    assert step(state=None) == -3 and b'nbasr_ctc_beam_stream_timed_step: NULL pointer' in _err(lib)
    assert step(c_frames=None) == -3 and step(p_frames=None) == -3 and step(usage=None) == -3
    assert step(width=33) == -1 and b'beam_width=33' in _err(lib)
    assert step(pool=0) == -1 and b'pool_nodes=0' in _err(lib)
    assert step(state=20) == -2 and b'8-byte aligned' in _err(lib)
    assert lib.nbasr_ctc_beam_stream_timed_init(None, 2, 12, 100, None) == -3 and b'NULL pointer' in _err(lib)
    assert lib.nbasr_ctc_beam_stream_timed_init(16, 2, 33, 100, None) == -1 and b'beam_width=33' in _err(lib)
    assert lib.nbasr_ctc_beam_stream_timed_init(12, 2, 12, 100, None) == -2 and b'8-byte aligned' in _err(lib)
    assert lib.nbasr_ctc_beam_stream_timed_finish(None, 16, 16, 16, 16, 4, 2, 12, 100, None) == -3 and b'NULL pointer' in _err(lib)
    assert lib.nbasr_ctc_beam_stream_timed_finish(16, 16, 16, None, 16, 4, 2, 12, 100, None) == -3
    assert lib.nbasr_ctc_beam_stream_timed_finish(16, 16, 16, 16, 16, 4, 2, 33, 100, None) == -1 and b'beam_width=33' in _err(lib)
    assert lib.nbasr_ctc_beam_stream_timed_finish(36, 16, 16, 16, 16, 4, 2, 12, 100, None) == -2 and b'8-byte aligned' in _err(lib)
    assert lib.nbasr_ctc_beam_stream_timed_init(None, 0, 12, 100, None) == 0


def test_timed_state_is_a_layout_of_its_own_and_the_untimed_one_is_unchanged():
    lib = hip.load_library()
    timed, plain = lib.nbasr_ctc_beam_stream_timed_state_bytes, lib.nbasr_ctc_beam_stream_state_bytes
    for width in (1, 7, 12, 32):
        assert plain(1, width, 100) == 64 + ((44 * width + 7) & ~7) + 100 * 8           # header, lanes, pool: as before this feature
        assert timed(1, width, 100) == 64 + 48 * width + 100 * 16                          # + p_best per lane, 16-byte nodes
        assert timed(1, width, 300) - timed(1, width, 100) == 200 * 16                     # the pool is the record's tail
        assert timed(5, width, 100) == 5 * timed(1, width, 100) and timed(1, width, 100) % 8 == 0
    assert timed(2, 33, 100) == 0 and timed(2, 12, 0) == 0 and timed(0, 12, 100) == 0
    assert hip.ctc_beam_stream_state_bytes(2, 12, 100) == plain(2, 12, 100)
    assert hip.ctc_beam_stream_state_bytes(2, 12, 100, timesteps=True) == timed(2, 12, 100)


def test_python_interface_keeps_its_positional_parameters():
    params = list(inspect.signature(ctc.beam_decode).parameters.values())
    assert [p.name for p in params[:5]] == ['log_probs', 'output_len', 'beam_width', 'blank', 'cutoff_top_n']
    assert [p.default for p in params[1:5]] == [None, 12, 0, 40]
    extra = params[5]
    assert extra.name == 'return_timesteps' and extra.kind is inspect.Parameter.KEYWORD_ONLY and extra.default is False
    init = inspect.signature(ctc.BeamSearchStream.__init__).parameters
    assert list(init)[1:7] == ['batch', 'beam_width', 'blank', 'cutoff_top_n', 'device', 'pool_nodes']
    assert init['timesteps'].default is False
