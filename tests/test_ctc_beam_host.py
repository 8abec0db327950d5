"""CTC prefix beam search without a GPU: constructor, INI class path, refusals before a launch, the GPU tests' float64
restatement on two cases worked out by hand, and the CPU side of their conditions (no near-tie, bounds under the cap)."""
import ctypes

import numpy as np
import pytest

from . import test_ctc_beam_gpu as G


def test_constructor_and_ini_class_path(tmp_path):
    from neuralmonkey_amd.config.builder import resolve_symbol
    from neuralmonkey_amd.decoders import CTCBeamSearchDecoder
    assert resolve_symbol("decoders.ctc_beam_search.CTCBeamSearchDecoder") is CTCBeamSearchDecoder
    model = G.load_wrapped(tmp_path, "cpu", 8, decoder_extra="merge_repeated_outputs=False")
    beam = model.runners[0].decoder
    parent = beam.parent_decoder
    assert isinstance(beam, CTCBeamSearchDecoder) and beam.beam_size == 8 and beam.vocabulary is parent.vocabulary
    assert beam.merge_repeated_outputs is False and beam.graph_safe_training(False) is False
    assert beam.train_loss.key == parent.train_loss.key and beam.runtime_loss.key == parent.runtime_loss.key
    assert {beam, parent, parent.encoder} <= set(model.runners[0].feedables)
    assert not [n for n in model.tf_manager.sessions[0].store.names() if n.startswith("beam/")]     # no variables
    assert CTCBeamSearchDecoder("merging", parent, 64, merge_repeated_outputs=True).merge_repeated_outputs is True
    for bad in (0, 65):
        with pytest.raises(ValueError, match="beam_size must be between 1 and 64"):
            CTCBeamSearchDecoder("bad{}".format(bad), parent, bad)


def test_binding_table_and_refusals_before_any_launch():
    from neuralmonkey_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert all(getattr(lib, name).argtypes == args for name, (_, args) in _lib.CTC_BEAM_SIGNATURES.items())
    small, large = lib.nm_ctc_beam_workspace_bytes(2, 4, 40, 1), lib.nm_ctc_beam_workspace_bytes(2, 4, 40, 64)
    assert 0 < small < large and lib.nm_ctc_beam_workspace_bytes(2, 4, 3, 64) < large     # short list clamped to K - 1
    buf, ibuf = (ctypes.c_float * 64)(), (ctypes.c_int32 * 64)()
    for beam, k, flen, ws_bytes, text in ((0, 5, ibuf, 1 << 20, b"beam_size must be between 1 and 64"),
                                          (65, 5, ibuf, 1 << 20, b"beam_size must be between"), (4, 1, ibuf, 1 << 20, b"K >= 2"),
                                          (4, 5, None, 1 << 20, b"null pointer"), (4, 5, ibuf, 16, b"workspace too small")):
        rc = lib.nm_ctc_beam_search(None, buf, 5, 20, 4, 2, k, flen, beam, 1, 2, ibuf, ibuf, buf, buf, ws_bytes)
        assert rc < 0 and b"nm_ctc_beam_search" in lib.nm_last_error() and text in lib.nm_last_error(), text


def test_restatement_on_the_hand_made_cases():
    two, aba = G.hand_made()
    outs, score, _, final = G.beam_search_ref(two, [2], 4, True)
    # prefix 'a': a a + a - + - a = 0.16 + 0.24 + 0.24; the empty prefix: - - = 0.36 (what greedy decoding follows)
    assert outs == [[0]] and abs(score[0] - np.log(0.64)) < 1e-7 and abs(final[0] - np.log(0.64 / 0.36)) < 1e-6
    assert G.beam_search_ref(two, [2], 1, True)[0] == [[]]                     # beam 1 keeps the empty prefix: 0.6 > 0.4
    for merge, want in ((False, [0, 0]), (True, [0])):
        outs, score, _, final = G.beam_search_ref(aba, [3], 4, merge)
        # 'a a' has the one alignment a - a = 0.729; 'a' sums aaa aa- a-- -aa --a -a- = 0.262
        assert outs == [want] and abs(score[0] - np.log(0.729)) < 1e-7 and abs(final[0] - np.log(0.729 / 0.262)) < 1e-6
    assert G.beam_search_ref(two, [0], 4, True)[:2] == ([[]], 0.0)             # no frame: nothing, score 0


def test_gpu_cases_have_no_near_tie_and_their_bounds_are_sound():
    assert {(c[3], c[4]) for c in G.CASES.values()} >= {(3, 64), (5, 4), (40, 1), (40, 16), (40, 17), (40, 64), (2003, 8)}
    for name in sorted(G.CASES):
        exp = G.expectations(name)
        assert G.make_case(name)[1][1:3].tolist() == [0, 1] and exp["outs"][1] == [] and exp["score"][1] == 0.0, name
        assert exp["cut_gap"].min() > G.MARGIN and exp["final_gap"].min() > G.MARGIN, name
        assert 0 < exp["unit"] <= exp["bound"] <= exp["cap"], name
        print("{}: unit {:.3g}, bound {:.3g}, cap {:.3g}".format(name, exp["unit"], exp["bound"], exp["cap"]))
