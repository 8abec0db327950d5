"""The sequence-labelling heads without a GPU: the reference's class paths through the config loader, its two tagging
configurations (tests/labeler.ini, tests/bert.ini) built from the committed archive, constructor signatures, the feed,
the shape and mask errors, the third binding table (include/nmhip_label.h) with its argument checks and coverage
ledger, the NumPy restatement against the fixtures the reference's own Python produced, LabelRunner's collection of
results and the CPU side of the GPU tests' bounds."""
import ctypes
import glob
import json
import os
import re
import tarfile

import numpy as np
import pytest

from . import label_ref as R
from . import labeler_models as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
GOLDEN = os.path.join(ROOT, "tests", "golden")
LISTS = os.path.join(GOLDEN, "labeler_signatures.json")
BUNDLE = os.path.join(GOLDEN, "reference_tests_labeler.tar.gz")
FIX = os.path.join(GOLDEN, "labeler")
FORWARD_CASES = ["labeler_plain", "labeler_hidden_relu", "labeler_two_encoders", "embeddings_labeler_transformer",
                 "embeddings_labeler_projected", "embeddings_labeler_frozen", "fd_gradients_labeler",
                 "fd_gradients_embeddings_labeler"]


def load_fixture(case):
    z = np.load(os.path.join(FIX, case + ".npz"))
    return z, json.loads(str(z["cfg"])), {k[2:]: z[k] for k in z.files if k.startswith("p/")}


# ---- through the config loader ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,runner_class", [("tagger", "runners.LabelRunner"),
                                               ("mlm", "runners.label_runner.LabelRunner")])
def test_ini_with_the_references_class_paths_builds(tmp_path, kind, runner_class):
    """Fails on a tree without the feature with SymbolNotShipped."""
    from neuralmonkey_amd.decoders import EmbeddingsLabeler, SequenceLabeler
    from neuralmonkey_amd.decoders.sequence_labeler import SequenceLabeler as same
    from neuralmonkey_amd.runners import LabelRunner
    from neuralmonkey_amd.runners.label_runner import LabelRunner as same_runner
    assert SequenceLabeler is same and LabelRunner is same_runner
    model, _ = M.load(tmp_path, kind, "cpu", runner_class=runner_class, runners="<runner>, <runner_xent>")
    runner = model.runners[0]
    dec = runner.decoder
    assert isinstance(runner, LabelRunner) and runner.loss_names == ["loss"] and runner.output_series == "tags"
    assert type(dec) is (SequenceLabeler if kind == "tagger" else EmbeddingsLabeler)
    assert model.trainers[0].objectives[0].decoder is dec and model.runners[1].decoder is dec
    store = model.tf_manager.sessions[0].store
    mine = {n: tuple(store[n].shape) for n in store.names() if n.startswith("tagger/")}
    if kind == "tagger":
        assert mine == {"tagger/hidden_layer/kernel": (12, 10), "tagger/hidden_layer/bias": (10,),
                        "tagger/logits/kernel": (10, 8), "tagger/logits/bias": (8,)}
        assert dec.activation_name == "tanh" and dec.hidden_dim == 10
    else:
        assert mine == {} and dec.embedded_sequence is dec.encoders[0].input_sequence   # width = embedding: no variable
        assert dec.vocabulary is dec.embedded_sequence.vocabulary
        assert dec.embedded_sequence in dec.get_dependencies()[0]
    assert dec.graph_safe_training(True) == dec.encoders[0].graph_safe_training(True)
    batch = next(iter(model.train_dataset.batches()))
    fd = dec.feed_dict(batch, train=True)
    assert fd[dec.train_tokens].shape[0] == len(batch) and fd[dec.train_tokens].dtype == np.int32
    assert dec.train_token_count(type("Ctx", (), {"fed": lambda self, p: fd[p]})()) == float(
        (fd[dec.train_tokens] != 0).sum())
    from neuralmonkey_amd.dataset import Dataset
    bare = dec.feed_dict(Dataset("no_targets", series={"source": list(batch.get_series("source"))}), train=True)
    assert dec.train_tokens not in bare                          # no error without targets: the reference has none


@pytest.fixture(scope="module")
def ref_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("reference_tests_labeler")
    with tarfile.open(BUNDLE) as tar:
        tar.extractall(root)
    return str(root)


def glorot_limit(shape):
    return float(np.sqrt(6.0 / (shape[0] + shape[-1])))


def test_labeler_ini_builds_unmodified(ref_root):
    from neuralmonkey_amd.decoders import SequenceLabeler
    from neuralmonkey_amd.runners import LabelRunner
    from neuralmonkey_amd.trainers.delayed_update_trainer import DelayedUpdateTrainer
    from .test_reference_inis import load_verbatim
    model = load_verbatim(ref_root, "labeler", device="cpu")
    dec = model.runners[0].decoder
    assert isinstance(model.runners[0], LabelRunner) and isinstance(dec, SequenceLabeler) and dec.name == "tagger"
    assert isinstance(model.trainers[0], DelayedUpdateTrainer) and model.trainers[0].objectives[0].decoder is dec
    assert model.trainers[0].objectives[0].name == "tagger - cost"
    assert dec.hidden_dim is None and dec.dropout_keep_prob == 0.5 and dec.activation_name == "relu"
    classes = len(dec.vocabulary)
    assert classes == 38                                          # 39 lines of factored_tag_vocab.tsv: header, 34 tags
    store = model.tf_manager.sessions[0].store
    mine = {n: tuple(store[n].shape) for n in store.names() if n.startswith("tagger/")}
    assert mine == {"tagger/logits/kernel": (16, classes), "tagger/logits/bias": (classes,)}    # 8 + 8 bidirectional
    w = store["tagger/logits/kernel"]
    lim = glorot_limit(w.shape)
    assert float(w.abs().max()) <= lim and float(w.abs().max()) > 0.8 * lim
    assert float(store["tagger/logits/bias"].abs().max()) == 0.0
    batch = next(iter(model.train_dataset.batches()))
    assert len(batch) == 10 and dec.feed_dict(batch, train=True)[dec.train_tokens].shape[0] == 10


def test_bert_ini_builds_unmodified(ref_root):
    from neuralmonkey_amd.decoders import EmbeddingsLabeler
    from neuralmonkey_amd.runners import LabelRunner, XentRunner
    from .test_reference_inis import load_verbatim
    model = load_verbatim(ref_root, "bert", device="cpu")
    xent, runner = model.runners
    dec = runner.decoder
    assert isinstance(xent, XentRunner) and isinstance(runner, LabelRunner) and xent.decoder is dec
    assert isinstance(dec, EmbeddingsLabeler) and dec.name == "labeler_bert" and dec.max_output_len == 20
    assert dec.train_embeddings and dec.embedded_sequence is dec.encoders[0].input_sequence
    store = model.tf_manager.sessions[0].store
    assert not [n for n in store.names() if n.startswith("labeler_bert/")]      # width 6 = embedding 6: no projection
    table = store[dec.embedded_sequence.embedding_matrix_name]
    assert tuple(table.shape) == (len(dec.vocabulary), 6)
    assert dec.graph_safe_training(True) is True                  # a Transformer encoder: the step is captured


def test_archive_members_are_the_references_bytes(ref_root):
    with tarfile.open(BUNDLE) as tar:
        names = [m.name for m in tar.getmembers()]
    assert {"tests/labeler.ini", "tests/bert.ini", "tests/data/factored_tag_vocab.tsv",
            "tests/data/factored_decoder_vocab.tsv", "tests/data/labeler/train.pcedt.tags",
            "tests/data/bert/train.pcedt.forms.mask"} <= set(names)
    assert not [n for n in names if n.endswith((".py", ".sh"))]
    if os.path.isdir(REF):
        for rel in names:
            with open(os.path.join(REF, rel), "rb") as a, open(os.path.join(ref_root, rel), "rb") as b:
                assert a.read() == b.read(), rel


# ---- signatures ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,name", [("decoders/sequence_labeler.py", "SequenceLabeler"),
                                       ("decoders/sequence_labeler.py", "EmbeddingsLabeler"),
                                       ("runners/label_runner.py", "LabelRunner")])
def test_constructor_parameters_are_the_references(path, name):
    from .test_reference_signatures import product_parameters, read_reference_parameters
    with open(LISTS, encoding="utf-8") as handle:
        want = [tuple(p) for p in json.load(handle)[path][name]]
    if os.path.isdir(REF):
        assert read_reference_parameters(path, name) == want
    assert product_parameters(path, name) == want


def test_constructor_defaults_and_type_checks():
    import inspect
    from neuralmonkey_amd import tf_shim
    from neuralmonkey_amd.decoders import EmbeddingsLabeler, SequenceLabeler
    from neuralmonkey_amd.model.sequence import EmbeddedSequence
    from neuralmonkey_amd.runners import LabelRunner
    from neuralmonkey_amd.runtime import reset_registry
    from neuralmonkey_amd.vocabulary import Vocabulary
    defaults = {k: p.default for k, p in inspect.signature(SequenceLabeler.__init__).parameters.items()}
    assert (defaults["max_output_len"], defaults["hidden_dim"], defaults["dropout_keep_prob"],
            defaults["add_start_symbol"], defaults["add_end_symbol"]) == (None, None, 1.0, False, False)
    assert defaults["activation"] is tf_shim.nn.relu
    assert inspect.signature(EmbeddingsLabeler.__init__).parameters["train_embeddings"].default is True
    reset_registry()
    seq = EmbeddedSequence("seq", Vocabulary(["a", "b"]), "source", 4)
    dec = SequenceLabeler("lab", [seq], Vocabulary(["x"]), "tags")
    assert dec.input_types == {"tags": str} and dec.input_shapes == {"tags": [None, None]}
    assert dec.states_dimension == 4 and dec.train_loss.key == dec.cost.key == dec.runtime_loss.key
    with pytest.raises(TypeError):
        SequenceLabeler("lab2", seq, Vocabulary(["x"]), "tags")               # encoders is a list
    with pytest.raises(TypeError):
        LabelRunner("tags", dec, postprocess="no")
    with pytest.raises(NotImplementedError, match="activation"):
        SequenceLabeler("lab3", [seq], Vocabulary(["x"]), "tags", hidden_dim=3, activation=len)
    assert LabelRunner("tags", dec).decoder_data_id == "tags"


# ---- the feed -----------------------------------------------------------------------------------------------------------
def test_feed_ids_with_start_end_and_max_length_equal_the_references():
    from neuralmonkey_amd.dataset import Dataset
    from neuralmonkey_amd.decoders import SequenceLabeler
    from neuralmonkey_amd.model.sequence import EmbeddedSequence
    from neuralmonkey_amd.runtime import reset_registry
    from neuralmonkey_amd.vocabulary import Vocabulary
    z, cfg, _ = load_fixture("labeler_feed")
    assert cfg["max_output_len"] == 4 and cfg["add_start_symbol"] and cfg["add_end_symbol"]
    reset_registry()
    words = lambda n: Vocabulary(["w{}".format(i) for i in range(n)])
    seq = EmbeddedSequence("encoder_input", words(cfg["src_vocab"]), "source", cfg["emb"])
    dec = SequenceLabeler("tagger", [seq], words(cfg["tag_vocab"]), "tags", max_output_len=cfg["max_output_len"],
                          add_start_symbol=True, add_end_symbol=True)
    tags = [str(s).split() for s in z["in/tags"]]
    assert any(len(t) > 4 for t in tags) and any(len(t) < 3 for t in tags)       # one is cut, one keeps its </s>
    fd = dec.feed_dict(Dataset("fixture", series={"tags": tags}), train=True)
    assert np.array_equal(fd[dec.train_tokens], z["in/tgt_ids"])
    assert np.array_equal((fd[dec.train_tokens] != 0).astype(np.float32), z["out/train_mask"])


# ---- the two errors -----------------------------------------------------------------------------------------------------
def _two_sequence_model(second_series):
    from neuralmonkey_amd.dataset import Dataset
    from neuralmonkey_amd.decoders import SequenceLabeler
    from neuralmonkey_amd.model.sequence import EmbeddedSequence
    from neuralmonkey_amd.runtime import reset_registry
    from neuralmonkey_amd.tf_manager import TensorFlowManager
    from neuralmonkey_amd.vocabulary import Vocabulary
    reset_registry()
    vocab = Vocabulary(["a", "b", "c"])
    one = EmbeddedSequence("one", vocab, "source", 4)
    two = EmbeddedSequence("two", vocab, "other", 4)
    dec = SequenceLabeler("lab", [one, two], Vocabulary(["x", "y"]), "tags")
    tfm = TensorFlowManager(num_sessions=1, num_threads=1, device="cpu", seed=1)
    tfm.initialize_sessions()
    ds = Dataset("d", series={"source": [["a", "b", "c"], ["a"]], "other": second_series,
                              "tags": [["x", "y", "x"], ["y"]]})
    fd = {}
    for part in (one, two, dec):
        fd.update(part.feed_dict(ds, train=False))
    return tfm.sessions[0], dec, fd


@pytest.mark.parametrize("other", [[["a", "b"], ["c"]],                      # another width
                                   [["a", "b"], ["c", "a", "b"]]])            # the same width, other lengths
def test_unequal_encoder_masks_raise_the_references_message(other):
    sess, dec, fd = _two_sequence_model(other)
    with pytest.raises(ValueError, match="Encoders 'one' and 'two' does not have equal temporal masks."):
        sess.run({"mask": dec.input_mask}, fd)
    # a trainer stages every feedable's inputs on EVERY step, also before it replays a captured one: the check is there
    from neuralmonkey_amd.runtime import RunContext
    with pytest.raises(ValueError, match="does not have equal temporal masks"):
        dec.stage_inputs(RunContext(sess, fd))
    sess, dec, fd = _two_sequence_model([["c", "c", "b"], ["b"]])
    assert np.array_equal(np.asarray(sess.run({"mask": dec.input_mask}, fd)["mask"]), [[1, 1, 1], [1, 0, 0]])
    dec.stage_inputs(RunContext(sess, fd))


def test_target_width_other_than_the_encoders_steps_raises():
    from neuralmonkey_amd.dataset import Dataset
    sess, dec, fd = _two_sequence_model([["c", "c", "b"], ["b"]])
    fd.update(dec.feed_dict(Dataset("d", series={"tags": [["x", "y", "x", "y"], ["y"]]}), train=False))
    with pytest.raises(ValueError, match="'tags' are 4 wide, the encoder has 3 steps"):
        sess.run({"res": dec.train_loop_result}, fd)


# ---- the third binding table -------------------------------------------------------------------------------------------
def label_header_symbols():
    text = open(os.path.join(ROOT, "include", "nmhip_label.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nm_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


def test_label_header_matches_its_binding_table(lib):
    from neuralmonkey_amd import _lib
    from .test_abi import header_symbols
    from .test_ctc_host import ctc_header_symbols
    mine = label_header_symbols()
    assert mine == set(_lib.LABEL_SIGNATURES) and len(mine) == 3
    assert not mine & set(_lib.SIGNATURES) and not mine & set(_lib.CTC_SIGNATURES)
    assert not mine & header_symbols() and not mine & ctc_header_symbols()
    for name, (res, args) in _lib.LABEL_SIGNATURES.items():
        fn = getattr(lib, name)                                          # exported, and bound by load()
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_label_entry_points_validate_before_any_launch(lib):
    buf = (ctypes.c_float * 4096)()
    other = (ctypes.c_float * 4096)()
    ibuf = (ctypes.c_int32 * 64)()
    kmax = lib.nm_label_rows_max_classes()
    assert kmax == 1024

    def call(logits=buf, ld=8, rows=4, k=8, targets=ibuf, grad=0, loss=buf, logprobs=None, ldp=8, argmax=None,
             row_mask=None, labels=None):
        return lib.nm_label_rows(None, logits, ld, rows, k, targets, 0, None, grad, loss, logprobs, ldp, argmax,
                                 row_mask, 2, labels)
    for kwargs, text in (
            (dict(k=0), b"nm_label_rows: K = 0 classes, at least 1"),
            (dict(k=kmax + 1, ld=kmax + 1), b"nm_label_rows: K = 1025 classes above the packed kernel's maximum of 1024"),
            (dict(ld=7), b"nm_label_rows: ld 7 below K 8"),
            (dict(logprobs=other, ldp=7), b"nm_label_rows: ldp 7 below K 8"),
            (dict(targets=None, grad=1), b"nm_label_rows: write_grad without targets"),
            (dict(logprobs=buf), b"nm_label_rows: logprobs aliasing logits"),
            (dict(logprobs=ctypes.byref(buf, 4 * 20)), b"nm_label_rows: logprobs aliasing logits"),
            (dict(labels=ibuf), b"nm_label_rows: labels without row_mask"),
            (dict(rows=-1), b"nm_label_rows: bad row count"),
            (dict(logits=None), b"nm_label_rows: null pointer (logits)")):
        assert call(**kwargs) < 0 and text in lib.nm_last_error(), (kwargs, lib.nm_last_error())
    assert call(rows=0, logits=None, targets=None, loss=None) == 0             # rows == 0 is a no-op
    assert call(rows=0, logprobs=buf) == 0
    stats = lambda **kw: lib.nm_label_rows_from_stats(
        None, kw.get("logits", buf), kw.get("ld", 8), kw.get("rows", 4), kw.get("k", 8), ibuf, 0, kw.get("rmax", buf),
        buf, buf, None, kw.get("argmax", ibuf), kw.get("row_mask", buf), 2, kw.get("labels", None))
    assert stats(k=0) < 0 and b"nm_label_rows_from_stats: K = 0" in lib.nm_last_error()
    assert stats(ld=3) < 0 and b"nm_label_rows_from_stats: ld 3 below K 8" in lib.nm_last_error()
    assert stats(rmax=None) < 0 and b"loss_rows without logits, rmax or rlse" in lib.nm_last_error()
    assert stats(labels=ibuf, row_mask=None) < 0 and b"labels without row_mask or argmax" in lib.nm_last_error()
    assert stats(rows=0) == 0


def test_label_ledger_covers_its_header():
    from . import test_label_kernels_gpu as K
    from .test_pointwise_refs import ledger_problems
    assert ledger_problems(K.LEDGER, label_header_symbols()) == []
    assert not [s for s, e in K.LEDGER.items() if isinstance(e, tuple)]      # every entry point names a test that calls it
    gone = dict(K.LEDGER, nm_label_rows=K.HERE + "test_rows_was_deleted via ops.label_rows")
    assert any("no test test_rows_was_deleted" in p for p in ledger_problems(gone, label_header_symbols()))
    wrong = dict(K.LEDGER, nm_label_rows=K.HERE + "test_batch_of_pad_targets_only via ops.label_rows_max_classes")
    assert any("does not call ops.label_rows_max_classes" in p for p in ledger_problems(wrong, label_header_symbols()))


def test_kernels_of_the_label_head_do_not_spill(lib):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_resources
    finally:
        sys.path.pop(0)
    mine = {k: v for k, v in kernel_resources().items() if "label_rows_kernel" in k or "label_from_stats_kernel" in k}
    assert len(mine) == 6, sorted(mine)                            # five register counts of the packed kernel + one
    assert all(v["scratch"] == 0 and v["lds"] == 0 for v in mine.values())


# ---- the restatement against the reference's own numbers ---------------------------------------------------------------
def close(got, want, what, tol=1e-6):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(np.abs(want).max()), 1e-6)
    err = float(np.abs(got - want).max())
    assert err <= tol * scale, "{}: max |diff| {:.3e} (scale {:.3g})".format(what, err, scale)


def restate(z, cfg, params, dtype=np.float64):
    states = [z["out/enc{}_states".format(i)] for i in range(2 if cfg["second_encoder"] else 1)]
    return R.head(params, states, z["in/tgt_ids"], kind=cfg["head"], activation=cfg["activation"],
                  table=params["encoder_input/embedding_matrix_0"], train_embeddings=cfg["train_embeddings"],
                  dtype=dtype)


def test_fixture_directory_holds_the_issues_cases():
    have = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(FIX, "*.npz")))
    assert have == sorted(FORWARD_CASES + ["labeler_feed"])
    for case in FORWARD_CASES:
        z, cfg, _ = load_fixture(case)
        lens = (z["in/src_ids"] != 0).sum(1)
        assert 4 <= len(lens) <= 5 and 1 in lens and len(set(lens.tolist())) > 2          # ragged, a one-word sentence
        assert (z["in/tgt_tokens"] == "never-seen").any() and (z["in/tgt_ids"] == 3).any()    # an unknown tag -> <unk>
        assert (cfg["src_vocab"], cfg["emb"], cfg["rnn"]) == (17, 6, 5)
        assert cfg["head"] == "embeddings" or cfg["tag_vocab"] == 9


@pytest.mark.parametrize("case", FORWARD_CASES)
def test_restatement_reproduces_the_reference(case):
    z, cfg, params = load_fixture(case)
    out = restate(z, cfg, params)
    for key in ("states", "logits", "logprobs", "train_mask", "train_xents", "cost"):
        close(out[key], z["out/" + key], case + " " + key)
    assert np.array_equal(out["decoded"], z["out/decoded"])
    assert not (R.top_two_gap(z["out/logits"].reshape(-1, z["out/logits"].shape[2])) <= 1e-6).any()
    words = ["<pad>", "<s>", "</s>", "<unk>"] + ["w{}".format(i) for i in range(out["logits"].shape[2] - 4)]
    sents = R.runner_sentences(out["decoded"], z["out/input_mask"], words)
    assert [" ".join(s) for s in sents] == [str(s) for s in z["out/runner_sentences"]]
    close(z["out/runner_loss"], z["out/cost"], "runner loss")
    # the mask of the cost is the TARGETS' (an EmbeddingsLabeler's targets have holes the encoder's mask has not)
    if cfg["head"] == "embeddings":
        assert (z["out/train_mask"] != z["out/input_mask"]).any()


@pytest.mark.parametrize("case", ["fd_gradients_labeler", "fd_gradients_embeddings_labeler"])
def test_analytic_gradient_of_the_restatement_against_finite_differences_of_the_reference(case):
    """The head's variables only (the encoder's belong to other tests): the bounds of
    test_engine_gradients_against_the_reference_finite_differences."""
    z, cfg, params = load_fixture(case)
    grads = restate(z, cfg, params)["grads"]
    seen = 0
    for name, i, fd in zip([str(n) for n in z["fd/names"]], z["fd/index"], z["fd/value"]):
        if not name.startswith("tagger/"):
            continue
        got = float(grads[name].reshape(-1)[int(i)])
        assert abs(got - fd) <= 6e-3 + 2e-2 * abs(fd), (name, i, got, fd)
        seen += 1
    assert seen >= 8


# ---- LabelRunner ---------------------------------------------------------------------------------------------------------
def test_label_runner_collects_masked_labels():
    from neuralmonkey_amd.decoders import SequenceLabeler
    from neuralmonkey_amd.model.sequence import EmbeddedSequence
    from neuralmonkey_amd.runners import LabelRunner
    from neuralmonkey_amd.runtime import reset_registry
    from neuralmonkey_amd.vocabulary import Vocabulary
    reset_registry()
    seq = EmbeddedSequence("seq", Vocabulary(["a"]), "source", 4)
    dec = SequenceLabeler("lab", [seq], Vocabulary(["N", "V"]), "tags")          # ids 4, 5
    runner = LabelRunner("tags", dec, postprocess=lambda sents: [[w.lower() for w in s] for s in sents])
    assert set(runner.fetches) == {"labels", "loss"} and runner.loss_names == ["loss"]
    labels = np.array([[4, 5, 5], [5, 2, 2], [2, 2, 2], [0, 4, 2]], np.int32)     # masked positions arrive as </s>
    ex = runner.get_executable(compute_losses=True, summaries=False, num_sessions=1)
    ex.collect_results([{"labels": labels, "loss": np.float32(1.5)}])
    assert ex.result.outputs["tags"] == [["n", "v", "v"], ["v"], [], ["<pad>", "n"]]
    assert ex.result.losses == {"tags/loss": 1.5} and ex.result.size == 4
    plain = LabelRunner("tags", dec).get_executable(compute_losses=False, summaries=False, num_sessions=1)
    fetches, _ = plain.next_to_execute()
    assert fetches["loss"] == 0.0
    plain.collect_results([{"labels": labels, "loss": 0.0}])
    assert plain.result.outputs["tags"][0] == ["N", "V", "V"]
    with pytest.raises(ValueError, match="exactly 1 execution result, got 2"):
        ex.collect_results([{"labels": labels, "loss": 0.0}] * 2)
    # what the kernel computes on the device equals the reference's host arithmetic (label_runner.py:34-39)
    decoded = np.array([[4, 5, 5], [5, 4, 4]])
    mask = np.array([[1, 1, 1], [1, 0, 0]], np.float32)
    host = decoded - R.END
    host *= mask.astype(int)
    host += R.END
    assert np.array_equal(host, np.where(mask != 0, decoded, R.END))
    logits = np.eye(6)[[4, 5, 5, 5, 4, 4]]
    assert np.array_equal(R.rows(logits, None, row_mask=mask.reshape(-1))["labels"].reshape(2, 3), host)


# ---- the CPU side of the GPU tests' bounds -------------------------------------------------------------------------------
def test_gpu_bounds_are_positive_under_the_caps_and_no_row_is_a_near_tie():
    from . import test_label_kernels_gpu as K
    assert [(c[1], c[2]) for c in K.CASES.values()] == [(5, 1), (7, 2), (133, 43), (9, 64), (9, 65), (6, 257),
                                                         (5, 1024), (3, 1028)]
    assert K.CASES["k43_ld48"][3] == 48
    for name in K.CASES:
        x, t, mask, pad = K.make_case(name)
        _, rows, k, _ = K.CASES[name]
        exp = K.expectations(name)
        for key in ("loss", "grad", "logprobs"):
            if k == 1:           # log 1 and 1 - 1: identically zero in float64 and float32, the kernel must be exact
                assert exp["unit_" + key] == exp["bound_" + key] == 0.0 and not np.asarray(exp[key]).any()
                continue
            assert 0 < exp["bound_" + key] <= exp["cap_" + key], (name, key)
            assert exp["unit_" + key] <= exp["bound_" + key], (name, key)
        where = K.special_rows(rows)
        # the rows of equal values are exact ties with a defined answer; NO other row is within the margin
        gap, margin = R.top_two_gap(x), K.argmax_margin(x)
        near = gap <= margin
        assert exp["argmax"][where["equal"]] == 0 and (k == 1 or near[where["equal"]])
        near[where["equal"]] = False
        assert not near.any() or k == 1, name
        # what every case has to hold
        assert len(set(x[where["equal"]].tolist())) == 1
        assert t[where["pad"]] == pad and exp["loss"][where["pad"]] == 0.0 and not exp["grad"][where["pad"]].any()
        assert mask[where["masked"]] == 0.0 and t[where["masked"]] != pad and exp["labels"][where["masked"]] == K.MASKED
        fin = lambda r: x[r][np.isfinite(x[r])]
        assert 70 < fin(where["up"]).max() < 90 and -90 < fin(where["down"]).min() < -70        # every case: +-80
        # ... and a row that float32 cannot exponentiate without the maximum subtracted: exp overflows (+100) in
        # every case, every exponential of a row underflows (-110) from five rows on
        with np.errstate(over="ignore"):
            assert np.isinf(np.exp(fin(where["over"]))).any() and np.isfinite(np.exp(fin(where["up"])).sum())
        assert (rows < 5) == ("under" not in where)
        if "under" in where:
            assert not np.exp(fin(where["under"])).any() and np.exp(fin(where["down"])).all()
        assert t[where["over"]] != pad                                   # its loss and gradient count
        if k > 1:
            r = where["ninf"]
            assert np.isneginf(x[r]).any() and np.isfinite(x[r, t[r]]) and np.isfinite(exp["loss"][r])
            assert exp["loss"][where["masked"]] > 0.0
        assert np.isfinite(exp["loss"]).all()
