"""The CTC head without a GPU: constructor signatures against the reference's sources, an INI naming
decoders.ctc_decoder.CTCDecoder and encoders.numpy_stateful_filler.TemporalFiller built through the config loader,
TemporalFiller's feed, the label preparation, the second binding table (include/nmhip_ctc.h) with its argument checks
and coverage ledger, and the CPU side of the GPU tests' bounds."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from . import ctc_models as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
LISTS = os.path.join(ROOT, "tests", "golden", "ctc_signatures.json")


# ---- signatures ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,name", [("decoders/ctc_decoder.py", "CTCDecoder"),
                                       ("encoders/numpy_stateful_filler.py", "TemporalFiller")])
def test_constructor_parameters_are_the_references(path, name):
    """Names, order and which have defaults: the committed lists, which are the reference's wherever its tree is."""
    from .test_reference_signatures import product_parameters, read_reference_parameters
    with open(LISTS, encoding="utf-8") as handle:
        want = [tuple(p) for p in json.load(handle)[path][name]]
    if os.path.isdir(REF):
        assert read_reference_parameters(path, name) == want
    assert product_parameters(path, name) == want


def test_constructor_defaults_and_type_checks():
    import inspect
    from neuralmonkey_amd.decoders import CTCDecoder
    from neuralmonkey_amd.decoders.ctc_decoder import CTCDecoder as same
    from neuralmonkey_amd.encoders.numpy_stateful_filler import TemporalFiller
    from neuralmonkey_amd.runtime import reset_registry
    from neuralmonkey_amd.vocabulary import Vocabulary
    assert CTCDecoder is same
    defaults = {k: p.default for k, p in inspect.signature(CTCDecoder.__init__).parameters.items()}
    assert (defaults["max_length"], defaults["merge_repeated_targets"], defaults["merge_repeated_outputs"],
            defaults["beam_width"]) == (None, False, True, 1)
    reset_registry()
    filler = TemporalFiller("feats", "source", 39)
    assert filler.dimension == 39 and filler.dropout_keep_prob == 1.0 and filler.max_input_len is None
    assert filler.input_shapes == {"source": [None, None, 39]} and filler.input_types == {"source": np.float32}
    with pytest.raises(TypeError):
        TemporalFiller("feats2", "source", "39")
    dec = CTCDecoder("ctc", filler, Vocabulary(["a"]), "target", beam_width=4)        # constructs (signature parity)
    assert dec.input_types == {"target": str} and dec.input_shapes == {"target": [None, None]}
    with pytest.raises(NotImplementedError, match="ctc_beam_search_decoder"):
        dec.decoded.fn(dec, None)
    with pytest.raises(TypeError):
        CTCDecoder("ctc2", filler, Vocabulary(["a"]), "target", merge_repeated_targets="yes")


# ---- through the config loader ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", [("speech", 100), ("chars", 32)])
def test_ini_with_the_references_class_paths_builds(tmp_path, kind, dim):
    """Fails on a tree without the feature with SymbolNotShipped."""
    from neuralmonkey_amd.decoders import CTCDecoder
    from neuralmonkey_amd.encoders.numpy_stateful_filler import TemporalFiller
    model, _ = M.load(tmp_path, kind, "cpu")
    dec = model.runners[0].decoder
    assert isinstance(dec, CTCDecoder) and model.trainers[0].objectives[0].decoder is dec
    assert model.trainers[0].objectives[0].name == "decoder - cost"
    store = model.tf_manager.sessions[0].store
    mine = {n: tuple(store[n].shape) for n in store.names() if n.startswith("decoder/")}
    classes = len(M.WORDS) + 4 + 1                                      # the words, four special tokens, the blank
    assert mine == {"decoder/state_to_word_W": (dim, classes), "decoder/state_to_word_b": (classes,)}
    w = store["decoder/state_to_word_W"]
    assert float(w.min()) >= -0.5 and float(w.max()) < 0.5 and float(w.abs().max()) > 0.4
    assert float(store["decoder/state_to_word_b"].abs().max()) == 0.0
    if kind == "speech":
        assert isinstance(dec.encoder.input_sequence, TemporalFiller)
        assert not [n for n in store.names() if n.startswith(dec.encoder.input_sequence.name + "/")]   # no variables
    batch = next(iter(model.train_dataset.batches()))
    with pytest.raises(ValueError, match="You must feed reference sentences when training"):
        from neuralmonkey_amd.dataset import Dataset
        dec.feed_dict(Dataset("no_targets", series={"source": list(batch.get_series("source"))}), train=True)
    fd = dec.feed_dict(batch, train=True)
    assert fd[dec.train_tokens].shape[0] == len(batch) and fd[dec.train_tokens].dtype == np.int32


def test_beam_width_and_summed_loss_scaling(tmp_path):
    from neuralmonkey_amd.decoders import CTCDecoder
    model, _ = M.load(tmp_path, "speech", "cpu", decoder_extra="beam_width=8\nmerge_repeated_targets=True\nmax_length=3")
    dec = model.runners[0].decoder
    assert isinstance(dec, CTCDecoder) and dec.beam_width == 8 and dec.merge_repeated_targets and dec.max_length == 3
    assert dec.train_token_count(None) == 1.0           # weight / count: a summed loss is scaled by its weight alone
    assert dec.graph_safe_training(True) is False
    fd = dec.feed_dict(next(iter(model.train_dataset.batches())), train=True)
    assert fd[dec.train_tokens].shape[1] == 3           # truncated to max_length: no start symbol, no end symbol


# ---- TemporalFiller's feed ---------------------------------------------------------------------------------------------
def test_temporal_filler_pads_truncates_and_counts():
    from neuralmonkey_amd.dataset import Dataset
    from neuralmonkey_amd.encoders.numpy_stateful_filler import TemporalFiller
    from neuralmonkey_amd.runtime import reset_registry
    reset_registry()
    rng = np.random.default_rng(0)
    series = [rng.standard_normal((n, 5)).astype(np.float32) for n in (3, 7, 1, 5)]
    ds = Dataset("d", series={"feats": series})
    fd = TemporalFiller("f", "feats", 5).feed_dict(ds)
    part = TemporalFiller("g", "feats", 5, max_input_len=4)
    for filler, width, lens in ((None, 7, [3, 7, 1, 5]), (part, 4, [3, 4, 1, 4])):
        feed = fd if filler is None else filler.feed_dict(ds, train=True)
        states = [v for k, v in feed.items() if k.name.endswith("/temporal_states")][0]
        lengths = [v for k, v in feed.items() if k.name.endswith("/encoder_padding_lengths")][0]
        assert states.shape == (4, width, 5) and states.dtype == np.float32 and lengths.tolist() == lens
        for i, n in enumerate(lens):
            assert np.array_equal(states[i, :n], series[i][:n]) and not states[i, n:].any()
    assert part.feed_dict(ds, train=True)[part.train_mode] is True


# ---- label preparation ---------------------------------------------------------------------------------------------------
def test_label_preparation_matches_the_restatement():
    from neuralmonkey_amd.decoders.ctc_decoder import prepare_labels
    from neuralmonkey_amd.model.sequence import index_series
    from neuralmonkey_amd.vocabulary import Vocabulary
    from . import ctc_ref as R
    vocab = Vocabulary(["a", "b"])                                      # ids 4, 5
    sents = [["a", "a", "b"], [], ["b", "zzz", "zzz", "a", "a", "a"], ["b"]]
    for max_length in (None, 4):
        ids = index_series(sents, vocab, max_length, False, False)
        assert ids.shape == (4, 6 if max_length is None else 4)          # no start, no end symbol, truncated
        for merge in (False, True):
            labels, lens = prepare_labels(ids, merge)
            assert labels.dtype == np.int32 and lens.dtype == np.int32
            got = [labels[b, :lens[b]].tolist() for b in range(4)]
            assert got == R.prepare_labels(ids, merge)
            assert not any(0 in row for row in got) and labels.shape[1] == max(lens)
    ids = index_series(sents, vocab, None, False, False)
    assert prepare_labels(ids, True)[1].tolist() == [2, 0, 3, 1] and prepare_labels(ids, False)[1].tolist() == [3, 0, 6, 1]
    empty, lens = prepare_labels(np.zeros((3, 0), np.int32), True)
    assert empty.shape == (3, 0) and lens.tolist() == [0, 0, 0]


# ---- the second binding table ---------------------------------------------------------------------------------------------
def ctc_header_symbols():
    text = open(os.path.join(ROOT, "include", "nmhip_ctc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nm_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


def test_ctc_header_matches_its_binding_table(lib):
    from neuralmonkey_amd import _lib
    from .test_abi import header_symbols
    assert ctc_header_symbols() == set(_lib.CTC_SIGNATURES) and len(_lib.CTC_SIGNATURES) >= 4
    assert not set(_lib.CTC_SIGNATURES) & set(_lib.SIGNATURES) and not ctc_header_symbols() & header_symbols()
    for name, (res, args) in _lib.CTC_SIGNATURES.items():
        fn = getattr(lib, name)                                          # exported, and bound by load()
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_ctc_entry_points_validate_before_any_launch(lib):
    buf = (ctypes.c_float * 256)()
    ibuf = (ctypes.c_int32 * 64)()
    assert lib.nm_ctc_workspace_bytes(-1, 4, 2) < 0
    small, large = lib.nm_ctc_workspace_bytes(2, 4, 0), lib.nm_ctc_workspace_bytes(2, 4, 3)
    assert 0 < small < large and large >= 4 * (2 * 2 * 4 * 7 + 2 * 4)      # alpha and beta [B, T, 2 Lmax + 1] at least
    rc = lib.nm_ctc_loss_fwd(None, None, 5, 20, 4, 2, 5, ibuf, 3, ibuf, ibuf, 1, buf, buf, buf, 1 << 20)
    assert rc < 0 and b"nm_ctc_loss_fwd: null pointer" in lib.nm_last_error()
    rc = lib.nm_ctc_loss_fwd(None, buf, 5, 20, 4, 2, 5, None, 3, ibuf, ibuf, 1, buf, buf, buf, 1 << 20)
    assert rc < 0 and b"nm_ctc_loss_fwd: null pointer (labels)" in lib.nm_last_error()
    rc = lib.nm_ctc_loss_fwd(None, buf, 5, 20, 4, -2, 5, ibuf, 3, ibuf, ibuf, 1, buf, buf, buf, 1 << 20)
    assert rc < 0 and b"nm_ctc_loss_fwd: negative size" in lib.nm_last_error()
    rc = lib.nm_ctc_loss_fwd(None, buf, 5, 20, 4, 2, 5, ibuf, 3, ibuf, ibuf, 1, buf, buf, buf, 16)
    assert rc < 0 and b"workspace too small" in lib.nm_last_error()
    rc = lib.nm_ctc_loss_fwd(None, buf, 5, 20, 4, 2, 5, ibuf, 5000, ibuf, ibuf, 1, buf, buf, buf, 1 << 20)
    assert rc < 0 and b"labels per sentence" in lib.nm_last_error()
    rc = lib.nm_ctc_loss_bwd(None, buf, 5, 20, 4, 2, 5, ibuf, 3, ibuf, ibuf, None, None, 5, 20, buf, 1 << 20)
    assert rc < 0 and b"nm_ctc_loss_bwd: null pointer" in lib.nm_last_error()
    rc = lib.nm_ctc_loss_bwd(None, buf, 5, 20, 4, 2, 5, ibuf, 3, ibuf, ibuf, None, buf, -5, 20, buf, 1 << 20)
    assert rc < 0 and b"nm_ctc_loss_bwd: negative stride" in lib.nm_last_error()
    assert lib.nm_ctc_loss_bwd(None, None, 5, 20, 0, 2, 5, None, 3, None, None, None, None, 5, 20, None, 0) == 0   # no frame
    rc = lib.nm_ctc_greedy(None, buf, 5, 20, 4, 2, 5, None, 1, 2, ibuf, ibuf, buf, 1 << 20)
    assert rc < 0 and b"nm_ctc_greedy: null pointer" in lib.nm_last_error()
    rc = lib.nm_ctc_greedy(None, buf, 5, 20, 4, 2, 0, ibuf, 1, 2, ibuf, ibuf, buf, 1 << 20)
    assert rc < 0 and b"nm_ctc_greedy: negative size" in lib.nm_last_error()
    rc = lib.nm_ctc_mask_lengths(None, None, 4, 2, 4, ibuf)
    assert rc < 0 and b"nm_ctc_mask_lengths: null pointer" in lib.nm_last_error()
    rc = lib.nm_ctc_mask_lengths(None, buf, 3, 2, 4, ibuf)
    assert rc < 0 and b"nm_ctc_mask_lengths: bad shape" in lib.nm_last_error()


def test_ctc_ledger_covers_its_header():
    from . import test_ctc_kernels_gpu as K
    from .test_pointwise_refs import NO_KERNEL_ALLOWED, ledger_problems
    assert ledger_problems(K.LEDGER, ctc_header_symbols()) == []
    excused = [s for s, e in K.LEDGER.items() if isinstance(e, tuple)]
    assert excused == ["nm_ctc_workspace_bytes"] and all(NO_KERNEL_ALLOWED.match(s) for s in excused)
    gone = dict(K.LEDGER, nm_ctc_greedy=K.HERE + "test_greedy_was_deleted via ops.ctc_greedy")
    assert any("no test test_greedy_was_deleted" in p for p in ledger_problems(gone, ctc_header_symbols()))
    wrong = dict(K.LEDGER, nm_ctc_greedy=K.HERE + "test_loss_and_gradient_in_place via ops.ctc_greedy")
    assert any("does not call ops.ctc_greedy" in p for p in ledger_problems(wrong, ctc_header_symbols()))


def test_kernels_of_the_ctc_head_do_not_spill(lib):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_resources
    finally:
        sys.path.pop(0)
    mine = {k: v for k, v in kernel_resources().items() if "ctc_" in k}
    assert len(mine) == 6, sorted(mine)
    assert all(v["scratch"] == 0 for v in mine.values())


# ---- the CPU side of the GPU tests' bounds -------------------------------------------------------------------------------
def test_gpu_bounds_are_positive_under_the_caps_and_no_frame_is_a_near_tie():
    from . import ctc_ref as R
    from . import test_ctc_kernels_gpu as K
    assert {c[3] for c in K.CASES.values()} == {3, 40, 32001} and {c[5] for c in K.CASES.values()} == {True, False}
    assert any(2 * c[4] + 1 > 1024 for c in K.CASES.values())
    for name in sorted(K.CASES):
        logits, labels, frame_lens, merge = K.make_case(name)
        exp = K.expectations(name)
        assert 0 < exp["bound_loss"] <= exp["cap_loss"] and 0 < exp["bound_grad"] <= exp["cap_grad"], name
        # the float32 restatement itself stays inside the bound it defines
        assert exp["unit_loss"] <= exp["bound_loss"] and exp["unit_grad"] <= exp["bound_grad"], name
        assert not (R.top_two_gap(logits) <= K.greedy_margin(logits)).any(), name
        lens = [len(l) for l in labels]
        assert 0 in lens and 1 in frame_lens.tolist() and len(set(frame_lens.tolist())) > 2, name
        # (repeated labels everywhere but where the targets were collapsed, which leaves none by construction)
        assert any(a == b for lab in labels for a, b in zip(lab, lab[1:])) != K.CASES[name][6], name
        assert any(not R.has_alignment(l, int(n), merge) for l, n in zip(labels, frame_lens)), name
