"""SequenceSplitter, the gradient-blocking views and the word2vec plug-in without a GPU: constructor and function
signatures against the reference's, tests/language-model.ini verbatim from the committed archive (and the archive's
bytes), ``Word2Vec`` on the reference's tests/data/sample.w2v, and the splitter's refusals, sizes and declared variables
against what the reference's own module created (tests/golden/sequence_split, make_sequence_split_golden.py)."""
import json
import os
import tarfile

import numpy as np
import pytest

from .test_reference_inis import REF        # noqa: E402  (the reference tree, where there is one)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BUNDLE = os.path.join(GOLDEN, "reference_tests_language_model.tar.gz")
LISTS = os.path.join(GOLDEN, "sequence_split_signatures.json")
FIX = os.path.join(GOLDEN, "sequence_split")
SPLIT_CASES = ["split_plain", "split_projected_relu", "split_projected_tanh", "split_projected_linear"]


@pytest.fixture(scope="module")
def lm_root(tmp_path_factory):
    """tests/language-model.ini and tests/data/sample.w2v, plus the corpora of the first archive."""
    root = tmp_path_factory.mktemp("reference_tests_language_model")
    for bundle in (os.path.join(GOLDEN, "reference_tests.tar.gz"), BUNDLE):
        with tarfile.open(bundle) as tar:
            tar.extractall(root)
    return str(root)


def sample_rows(lm_root):
    """(words, float64 rows) of sample.w2v, read here line by line."""
    with open(os.path.join(lm_root, "tests", "data", "sample.w2v"), encoding="utf-8") as handle:
        count, width = (int(x) for x in next(handle).split())
        lines = [line.split() for line in handle]
    assert len(lines) == count == 19 and width == 5
    return [f[0] for f in lines], np.asarray([[float(x) for x in f[1:]] for f in lines], np.float64)


# ---- signatures ---------------------------------------------------------------------------------------------------------
SIGNATURES = [("model/sequence_split.py", "SequenceSplitter"), ("model/gradient_blocking.py", "StatefulView"),
              ("model/gradient_blocking.py", "TemporalStatefulView"), ("model/gradient_blocking.py", "SpatialStatefulView"),
              ("util/word2vec.py", "Word2Vec"), ("util/word2vec.py", "get_word2vec_initializer"),
              ("util/word2vec.py", "word2vec_vocabulary")]


@pytest.mark.parametrize("path,name", SIGNATURES)
def test_parameters_are_the_references(path, name):
    from .test_reference_signatures import product_parameters, read_reference_parameters
    with open(LISTS, encoding="utf-8") as handle:
        want = [tuple(p) for p in json.load(handle)[path][name]]
    if os.path.isdir(REF):
        assert read_reference_parameters(path, name) == want
    assert product_parameters(path, name) == want


# ---- tests/language-model.ini ---------------------------------------------------------------------------------------------
def test_archive_members_are_the_references_bytes(lm_root):
    with tarfile.open(BUNDLE) as tar:
        names = [m.name for m in tar.getmembers()]
    assert set(names) == {"tests/language-model.ini", "tests/data/sample.w2v"} and len(names) == 2
    assert os.path.getsize(os.path.join(lm_root, "tests", "data", "sample.w2v")) == 984
    assert os.path.getsize(BUNDLE) < 4 * 1024
    if os.path.isdir(REF):
        for rel in names:
            with open(os.path.join(REF, rel), "rb") as a, open(os.path.join(lm_root, rel), "rb") as b:
                assert a.read() == b.read(), rel


def test_language_model_ini_builds_unmodified(lm_root):
    """Fails on a tree without the feature with SymbolNotShipped (util.word2vec.Word2Vec).  The decoder's vocabulary is
    the word2vec one: the four special tokens and the file's words that are none of them -- 19 entries of which two,
    ``</s>`` and ``<unk>``, are special, so 4 + 17."""
    from neuralmonkey_amd.config.builder import OutOfScope
    from neuralmonkey_amd.decoders import Decoder
    from neuralmonkey_amd.runners import XentRunner
    from neuralmonkey_amd.vocabulary import SPECIAL_TOKENS
    from .test_reference_inis import load_verbatim
    with pytest.warns(UserWarning, match="evaluators.PerplexityEvaluator is not part of this engine"):
        model = load_verbatim(lm_root, "language-model", device="cpu")
    runner, = model.runners
    dec = runner.decoder
    assert isinstance(runner, XentRunner) and runner.output_series == "xents"
    assert isinstance(dec, Decoder) and dec.encoders == [] and dec.name == "decoder"
    words, rows = sample_rows(lm_root)
    ordinary = [w for w in words if w not in SPECIAL_TOKENS]
    assert len(words) - len(ordinary) == 2
    assert list(dec.vocabulary.index_to_word) == SPECIAL_TOKENS + ordinary and len(dec.vocabulary) == 4 + len(ordinary)
    (series, data_id, evaluator), = model.evaluation
    assert (series, data_id) == ("xents", "target")
    assert isinstance(evaluator, OutOfScope) and evaluator.symbol == "evaluators.PerplexityEvaluator"
    assert evaluator.name == "perplexity"
    assert model.trainers[0].objectives[0].decoder is dec
    # the embedding variable is the file's rows, rounded to float32 once
    table = model.tf_manager.sessions[0].store["decoder/word_embeddings"].numpy()
    assert table.shape == (len(dec.vocabulary), 5) and table.dtype == np.float32
    assert np.array_equal(table[4:], np.asarray([rows[words.index(w)] for w in ordinary]).astype(np.float32))
    assert np.array_equal(table[2], rows[words.index("</s>")].astype(np.float32))
    assert np.array_equal(table[3], rows[words.index("<unk>")].astype(np.float32))
    assert not table[:2].any()


# ---- Word2Vec --------------------------------------------------------------------------------------------------------------
def test_word2vec_on_the_references_sample(lm_root):
    from neuralmonkey_amd.util.word2vec import Word2Vec, get_word2vec_initializer, word2vec_vocabulary
    from neuralmonkey_amd.vocabulary import END_TOKEN_INDEX, UNK_TOKEN_INDEX, Vocabulary
    w2v = Word2Vec(os.path.join(lm_root, "tests", "data", "sample.w2v"))
    words, rows = sample_rows(lm_root)
    vocab = w2v.vocabulary
    assert isinstance(vocab, Vocabulary) and word2vec_vocabulary(w2v) is vocab
    assert list(vocab.index_to_word) == ["<pad>", "<s>", "</s>", "<unk>", "the", ",", ".", "to", "of", "and", "a", "in",
                                         "&quot;", "@-@", "&apos;s", "that", "for", "is", "on", "it", "was"]
    emb = w2v.embeddings
    assert emb.dtype == np.float64 and emb.shape == (len(vocab), 5)
    assert (END_TOKEN_INDEX, UNK_TOKEN_INDEX) == (2, 3)
    assert np.array_equal(emb[2], rows[words.index("</s>")]) and np.array_equal(emb[3], rows[words.index("<unk>")])
    assert emb[3].tolist() == [0.250020, -0.214136, -0.157372, 0.202529, -0.043517]
    assert not emb[0].any() and not emb[1].any()
    for i, word in enumerate(vocab.index_to_word[4:], 4):
        assert np.array_equal(emb[i], rows[words.index(word)]), word
    init = get_word2vec_initializer(w2v)
    assert init(np.random.default_rng(0), (21, 5)) is emb and init(None, [21, 5]) is emb
    with pytest.raises(ValueError) as info:
        init(None, (20, 5))
    assert str(info.value) == ("Shapes of model and word2vec embeddings do not match. "
                               "Word2Vec shape: (21, 5), Should have been: [20, 5]")
    with pytest.raises(TypeError):
        Word2Vec(5)
    with pytest.raises(TypeError):
        get_word2vec_initializer("sample.w2v")


def test_word2vec_initializer_is_one_of_this_packages(lm_root):
    """Parameterized.declare hands a two-argument callable (rng, shape) through as it is; the store rounds once."""
    from neuralmonkey_amd.model.model_part import _is_rng_init
    from neuralmonkey_amd.model.sequence import EmbeddedSequence
    from neuralmonkey_amd.runtime import reset_registry
    from neuralmonkey_amd.util.word2vec import Word2Vec, get_word2vec_initializer
    from neuralmonkey_amd.variables import VariableStore
    reset_registry()
    w2v = Word2Vec(os.path.join(lm_root, "tests", "data", "sample.w2v"))
    init = get_word2vec_initializer(w2v)
    assert _is_rng_init(init)
    seq = EmbeddedSequence("seq", w2v.vocabulary, "source", 5, initializers=[("embedding_matrix_0", init)])
    store = VariableStore("cpu", seed=3)
    seq.declare_variables(store)
    store.finalize()
    assert np.array_equal(store["seq/embedding_matrix_0"].numpy(), w2v.embeddings.astype(np.float32))
    reset_registry()
    wrong = EmbeddedSequence("seq", w2v.vocabulary, "source", 4, initializers=[("embedding_matrix_0", init)])
    store = VariableStore("cpu", seed=3)
    wrong.declare_variables(store)
    with pytest.raises(ValueError, match="Shapes of model and word2vec embeddings do not match."):
        store.finalize()


# ---- SequenceSplitter on the host -----------------------------------------------------------------------------------------
def _words(n):
    from neuralmonkey_amd.vocabulary import Vocabulary
    return Vocabulary(["w{}".format(i) for i in range(n)])


def _sequence(width=12):
    from neuralmonkey_amd.model.sequence import EmbeddedSequence
    from neuralmonkey_amd.runtime import reset_registry
    reset_registry()
    return EmbeddedSequence("input", _words(11), "source", width)


def test_splitter_refusals_carry_the_references_words():
    from neuralmonkey_amd import tf_shim
    from neuralmonkey_amd.model.sequence_split import SequenceSplitter
    from neuralmonkey_amd.variables import VariableStore
    seq = _sequence(12)
    with pytest.raises(ValueError) as info:
        SequenceSplitter("s", seq, 5, projection_size=12)
    assert str(info.value) == "Dimension of projection (12) must be dividable by the given factor (5)."
    bad = SequenceSplitter("s", seq, 5)                       # the width is the parent's: checked where it is known
    for use in (lambda: bad.dimension, lambda: bad.declare_variables(VariableStore("cpu"))):
        with pytest.raises(ValueError) as info:
            use()
        assert str(info.value) == "Dimension of the tensor (12) must be dividable by the given factor (5)."
    for factor in (0, -2):
        with pytest.raises(ValueError, match="factor"):
            SequenceSplitter("s", seq, factor)
    with pytest.raises(NotImplementedError, match="activation"):
        SequenceSplitter("s", seq, 2, projection_size=8, projection_activation=np.tanh)
    with pytest.raises(NotImplementedError, match="activation"):
        SequenceSplitter("s", seq, 2, projection_size=8, projection_activation=abs)
    for wrong in (dict(parent="input", factor=2), dict(parent=seq, factor="2"), dict(parent=seq, factor=2.0),
                  dict(parent=seq, factor=2, projection_size="8")):
        with pytest.raises(TypeError):
            SequenceSplitter("s", **wrong)
    for act in (None, tf_shim.nn.relu, tf_shim.tanh, tf_shim.identity):
        SequenceSplitter("s", seq, 2, projection_size=8, projection_activation=act)


@pytest.mark.parametrize("case", SPLIT_CASES)
def test_splitter_sizes_and_variables_are_the_references(case):
    from neuralmonkey_amd import tf_shim
    from neuralmonkey_amd.model.model_part import ModelPart
    from neuralmonkey_amd.model.sequence_split import SequenceSplitter
    from neuralmonkey_amd.model.stateful import TemporalStateful
    from neuralmonkey_amd.tf_bundle import tf_shape
    from neuralmonkey_amd.variables import VariableStore
    z = np.load(os.path.join(FIX, case + ".npz"))
    cfg = json.loads(str(z["cfg"]))
    seq = _sequence(cfg["emb"])
    act = {None: None, "relu": tf_shim.nn.relu, "tanh": tf_shim.tanh}[cfg["activation"]]
    split = SequenceSplitter("splitter", seq, cfg["factor"], projection_size=cfg["projection_size"],
                             projection_activation=act)
    assert isinstance(split, TemporalStateful) and isinstance(split, ModelPart)
    assert split.dimension == int(z["out/dimension"]) == z["out/temporal_states"].shape[2]
    assert split.dimension == (cfg["projection_size"] or cfg["emb"]) // cfg["factor"]
    assert [str(d) for d in z["out/dependencies"]] == [d for d in split.dependencies]
    feedables, parameterizeds = split.get_dependencies()
    assert seq in feedables and seq in parameterizeds and split in feedables and split in parameterizeds
    store = VariableStore("cpu")
    seq.declare_variables(store)
    split.declare_variables(store)
    mine = {n: list(tf_shape(n, s.shape)) for n, s in store.specs.items()}
    theirs = {str(n): list(z["p/" + str(n)].shape) for n in z["var_order"]}
    assert mine == theirs
    assert ("splitter/dense/kernel" in mine) == (cfg["projection_size"] is not None)
    if cfg["projection_size"] is not None:
        assert mine["splitter/dense/kernel"] == [cfg["emb"], cfg["projection_size"]]
        assert mine["splitter/dense/bias"] == [cfg["projection_size"]]
        store.seed = 7
        store.finalize()
        kernel, bias = store["splitter/dense/kernel"].numpy(), store["splitter/dense/bias"].numpy()
        limit = np.sqrt(6.0 / (cfg["emb"] + cfg["projection_size"]))               # glorot uniform, zeros
        assert np.abs(kernel).max() <= limit and np.abs(kernel).max() > 0.5 * limit and not bias.any()
    # the recorded forward pass is the projection followed by a plain reshape, the mask each entry `factor` times
    x = z["in/parent_states"].astype(np.float64)
    if cfg["projection_size"] is not None:
        x = x @ z["p/splitter/dense/kernel"].astype(np.float64) + z["p/splitter/dense/bias"].astype(np.float64)
        x = {None: lambda v: v, "relu": lambda v: np.maximum(v, 0), "tanh": np.tanh}[cfg["activation"]](x)
    bsz, steps, width = x.shape
    want = x.reshape(bsz, steps * cfg["factor"], width // cfg["factor"])
    assert np.abs(z["out/temporal_states"] - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    assert np.array_equal(z["out/temporal_mask"], np.repeat(z["in/parent_mask"], cfg["factor"], axis=1))
    assert np.array_equal(z["out/lengths"], z["in/parent_mask"].sum(1).astype(np.int32) * cfg["factor"])
    assert z["out/lengths"].dtype == np.int32


# ---- the splitter's binding table -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


def test_split_header_matches_its_binding_table_and_refuses_before_any_launch(lib):
    import ctypes
    import re
    from neuralmonkey_amd import _lib
    from .test_abi import header_symbols
    from .test_pool_host import pool_header_symbols
    text = open(os.path.join(os.path.dirname(HERE), "include", "nmhip_split.h")).read()
    assert "sequence_split.py:60-66" in text and "stateful.py:55-62" in text             # the lines it replaces
    mine = set(re.findall(r"\b(nm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert mine == set(_lib.SPLIT_SIGNATURES) == {"nm_split_mask"}
    assert not mine & header_symbols() and not mine & pool_header_symbols() and not mine & set(_lib.POOL_SIGNATURES)
    for name, (res, args) in _lib.SPLIT_SIGNATURES.items():
        fn = getattr(lib, name)                                          # exported, and bound by load()
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    # host buffers and a null stream: a call that got as far as a launch would fault or fail differently
    buf, other, ibuf = (ctypes.c_float * 4096)(), (ctypes.c_float * 4096)(), (ctypes.c_int32 * 64)()

    def call(mask=buf, b=2, t=3, factor=2, out=other, lengths=ibuf):
        return lib.nm_split_mask(None, mask, b, t, factor, out, lengths)
    for kwargs, message in ((dict(b=0), b"nm_split_mask: bad sizes B 0, T 3, factor 2"), (dict(t=0), b"bad sizes"),
                            (dict(factor=0), b"bad sizes"), (dict(factor=-1), b"bad sizes"),
                            (dict(t=1 << 24), b"beyond the grid or the exact fp32 row sum"),
                            (dict(t=1 << 20, factor=1 << 12), b"beyond the grid"), (dict(b=1 << 31), b"beyond the grid"),
                            (dict(mask=None), b"nm_split_mask: null pointer"), (dict(out=None), b"null pointer"),
                            (dict(lengths=None), b"null pointer"), (dict(out=buf), b"nm_split_mask: out_mask aliasing mask"),
                            (dict(out=ctypes.byref(buf, 4 * 5)), b"out_mask aliasing mask")):
        assert call(**kwargs) < 0 and message in lib.nm_last_error(), (kwargs, lib.nm_last_error())


def test_blocking_views_pass_the_viewed_parts_handles_through():
    from neuralmonkey_amd.encoders import SentenceEncoder, SequenceMaxPooling
    from neuralmonkey_amd.model import gradient_blocking as B
    from neuralmonkey_amd.runtime import part_reads, reset_registry
    reset_registry()
    enc = SentenceEncoder(name="encoder", vocabulary=_words(12), data_id="source", embedding_size=8, rnn_size=8)
    pool = SequenceMaxPooling("pool", enc)
    view, tview = B.StatefulView(pool), B.TemporalStatefulView(enc)
    assert view.output.key == pool.output.key and view.output_size == pool.output_size
    assert tview.temporal_states.key == enc.temporal_states.key and tview.temporal_mask.key == enc.temporal_mask.key
    assert tview.dimension == enc.dimension
    for v, part in ((view, pool), (tview, enc)):
        assert v.dependencies == ["_blocked_object"] and v._blocked_object is part      # pylint: disable=protected-access
        assert part in v.get_dependencies()[0] and part in v.get_dependencies()[1]
        assert v.graph_safe_training(True) == part.graph_safe_training(True)
        assert part_reads(v) == []                            # nothing waits for a gradient from a blocking view
    with pytest.raises(TypeError):
        B.StatefulView("pool")
    with pytest.raises(TypeError):
        B.SpatialStatefulView(blocked_object=enc)              # a temporal part is no spatial one

    class Ctx:                                                 # backward hands nothing on
        memo = {"backward_deferred": True}

        def defer_backward(self, *args):
            raise AssertionError("a blocking view handed a gradient on")
    assert view.backward(Ctx(), None, object()) is None and tview.backward(Ctx(), object()) is None
