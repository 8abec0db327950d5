"""The sentence-level heads without a GPU: the reference's class paths through the config loader and its two
configurations (tests/classifier.ini, tests/regressor.ini) built from the committed archive, constructor signatures and
argument checks, the fourth binding table (include/nmhip_pool.h) with its refusals, the NumPy restatement
(tests/pool_ref.py) against the fixtures the reference's own Python produced and against torch float64 autograd, the
order of deferred backward passes and the runners' collection of results."""
import ctypes
import glob
import json
import os
import re
import tarfile

import numpy as np
import pytest

from . import classifier_models as M
from . import pool_ref as R

from .test_reference_inis import REF        # noqa: E402  (the reference tree, where there is one)

ROOT = M.ROOT


# ---- through the config loader ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_root(tmp_path_factory):
    """tests/<name>.ini and tests/data: the committed archives, extracted (the parallel text and the encoder vocabulary
    the two configurations name are in the first archive)."""
    root = tmp_path_factory.mktemp("reference_tests_classifier")
    for bundle in (os.path.join(M.GOLDEN, "reference_tests.tar.gz"), M.BUNDLE):
        with tarfile.open(bundle) as tar:
            tar.extractall(root)
    return str(root)


def without_cnn_encoder(ref_root):
    """tests/classifier.ini with its [encoder_cnn] section and that entry of ``encoders=`` removed: SequenceCNNEncoder
    is not part of this engine."""
    text = open(os.path.join(ref_root, "tests", "classifier.ini")).read()
    edited, n = re.subn(r"\[encoder_cnn\]\n(?:[^\[\n][^\n]*\n)+\n", "", text)
    assert n == 1
    assert ", <encoder_cnn>]" in edited
    edited = edited.replace(", <encoder_cnn>]", "]")
    assert "encoder_cnn" not in edited
    with open(os.path.join(ref_root, "tests", "classifier_without_cnn.ini"), "w") as handle:
        handle.write(edited)
    return "classifier_without_cnn"


def test_regressor_ini_builds_unmodified(ref_root):
    """Fails on a tree without the feature with SymbolNotShipped."""
    from neuralmonkey_amd.decoders import SequenceRegressor
    from neuralmonkey_amd.runners import RegressionRunner
    from .test_reference_inis import load_verbatim
    model = load_verbatim(ref_root, "regressor", device="cpu")
    runner = model.runners[0]
    dec = runner.decoder
    assert isinstance(runner, RegressionRunner) and isinstance(dec, SequenceRegressor) and dec.name == "regressor"
    assert runner.loss_names == ["mse"] and runner.output_series == "regression" and runner.postprocess is None
    assert model.trainers[0].objectives[0].decoder is dec and model.trainers[0].objectives[0].name == "regressor - cost"
    store = model.tf_manager.sessions[0].store
    mine = {n: tuple(store[n].shape) for n in store.names() if n.startswith("regressor/")}
    assert mine == {"regressor/mlp/mlp_layer_0/kernel": (14, 10), "regressor/mlp/mlp_layer_0/bias": (10,),
                    "regressor/mlp/mlp_layer_1/kernel": (10, 5), "regressor/mlp/mlp_layer_1/bias": (5,),
                    "regressor/output_projection/kernel": (5, 1), "regressor/output_projection/bias": (1,)}
    batch = next(iter(model.train_dataset.batches()))
    fd = dec.feed_dict(batch, train=True)
    want = [float(row[0]) for row in batch.get_series("regression")]
    assert fd[dec.targets_placeholder].dtype == np.float32 and fd[dec.targets_placeholder].tolist() == want
    ctx = type("Ctx", (), {"fed": lambda self, p: fd[p]})()
    assert dec.train_token_count(ctx) == float(len(batch) * 1)
    assert dec.graph_safe_training(True) == dec.encoders[0].graph_safe_training(True)
    assert dec.input_types == {"regression": float} and dec.input_shapes == {"regression": [None]}


def test_classifier_ini_builds_without_its_cnn_encoder(ref_root):
    """Fails on a tree without the feature with SymbolNotShipped."""
    from neuralmonkey_amd.decoders import Classifier
    from neuralmonkey_amd.encoders import AttentiveEncoder, SentenceEncoder, SequenceMaxPooling
    from neuralmonkey_amd.model.gradient_reversal import StatefulView
    from neuralmonkey_amd.runners import GreedyRunner, LogitsRunner
    from .test_reference_inis import load_verbatim
    model = load_verbatim(ref_root, without_cnn_encoder(ref_root), device="cpu")
    greedy, logits = model.runners
    dec = greedy.decoder
    assert isinstance(greedy, GreedyRunner) and isinstance(logits, LogitsRunner) and logits.decoder is dec
    assert logits.normalize is True and logits.pick_index is None and logits.loss_names == ["train_loss", "runtime_loss"]
    assert isinstance(dec, Classifier) and dec.name == "decoder" and dec.layers == [10, 5] and dec.max_output_len == 1
    att, pool = dec.encoders
    assert isinstance(att, AttentiveEncoder) and isinstance(pool, SequenceMaxPooling)
    assert isinstance(att.input_sequence, SentenceEncoder) and pool.input_sequence is att.input_sequence
    assert (att.output_size, att.dimension, pool.output_size) == (13, 14, 14)
    main, adv = [o.decoder for o in model.trainers[0].objectives]
    assert main is dec and adv.name == "decoder_adv" and adv.layers == []        # (named after its section)
    view, = adv.encoders
    assert isinstance(view, StatefulView) and view.output_size == 14 and view.output.key == pool.output.key
    assert pool in adv.get_dependencies()[0] and att.input_sequence in adv.get_dependencies()[1]
    classes = len(dec.vocabulary)
    store = model.tf_manager.sessions[0].store
    mine = {n: tuple(store[n].shape) for n in store.names() if not n.startswith("sentence_encoder")}
    pre = "decoder/multilayer_perceptron/"
    assert mine == {"attentive_encoder/S1/kernel": (14, 9), "attentive_encoder/S2/kernel": (9, 5),
                    "attentive_encoder/output_projection/kernel": (70, 13),
                    "attentive_encoder/output_projection/bias": (13,),
                    pre + "deep_output_mlp/mlp_layer_0/kernel": (27, 10), pre + "deep_output_mlp/mlp_layer_0/bias": (10,),
                    pre + "deep_output_mlp/mlp_layer_1/kernel": (10, 5), pre + "deep_output_mlp/mlp_layer_1/bias": (5,),
                    pre + "classification_layer/kernel": (5, classes), pre + "classification_layer/bias": (classes,),
                    "decoder_adv/multilayer_perceptron/classification_layer/kernel": (14, classes),
                    "decoder_adv/multilayer_perceptron/classification_layer/bias": (classes,)}
    batch = next(iter(model.train_dataset.batches()))
    fd = dec.feed_dict(batch, train=True)
    ids = fd[dec.targets_placeholder]
    assert ids.dtype == np.int32 and ids.shape == (len(batch),)
    first = [[s[0]] for s in batch.get_series("classification")]
    assert ids.tolist() == dec.vocabulary.strings_to_indices(first)[:, 0].tolist() and ids.min() >= 4
    assert dec.graph_safe_training(True) == att.input_sequence.graph_safe_training(True)
    assert dec.train_loss.key == dec.runtime_loss.key == dec.cost.key
    assert dec.input_types == {"classification": str} and dec.input_shapes == {"classification": [None]}


def test_classifier_ini_as_it_is_names_the_one_missing_encoder(ref_root):
    from neuralmonkey_amd.config.builder import SymbolNotShipped
    from .test_reference_inis import load_verbatim
    with pytest.raises(Exception) as info:
        load_verbatim(ref_root, "classifier", device="cpu")
    chain, exc = [], info.value
    while exc is not None:
        chain.append(exc)
        exc = exc.__cause__ or exc.__context__
    assert any(isinstance(e, SymbolNotShipped) for e in chain) and "sequence_cnn_encoder" in str(info.value)


def test_archive_members_are_the_references_bytes(ref_root):
    with tarfile.open(M.BUNDLE) as tar:
        names = [m.name for m in tar.getmembers()]
    assert set(names) == {"tests/classifier.ini", "tests/regressor.ini", "tests/data/train.words",
                          "tests/data/val.words", "tests/data/classification.vocab", "tests/data/train.tc.counts",
                          "tests/data/val.tc.counts"}
    assert os.path.getsize(M.BUNDLE) < 16 * 1024
    if os.path.isdir(REF):
        for rel in names:
            with open(os.path.join(REF, rel), "rb") as a, open(os.path.join(ref_root, rel), "rb") as b:
                assert a.read() == b.read(), rel


# ---- signatures and argument checks --------------------------------------------------------------------------------------
SIGNATURES = [("encoders/pooling.py", "SequencePooling"), ("encoders/attentive.py", "AttentiveEncoder"),
              ("model/gradient_reversal.py", "StatefulView"), ("model/gradient_reversal.py", "TemporalStatefulView"),
              ("model/gradient_reversal.py", "SpatialStatefulView"), ("decoders/classifier.py", "Classifier"),
              ("decoders/sequence_regressor.py", "SequenceRegressor"), ("runners/logits_runner.py", "LogitsRunner"),
              ("runners/regression_runner.py", "RegressionRunner")]


@pytest.mark.parametrize("path,name", SIGNATURES)
def test_constructor_parameters_are_the_references(path, name):
    from .test_reference_signatures import product_parameters, read_reference_parameters
    with open(M.LISTS, encoding="utf-8") as handle:
        want = [tuple(p) for p in json.load(handle)[path][name]]
    if os.path.isdir(REF):
        assert read_reference_parameters(path, name) == want
    assert product_parameters(path, name) == want


def test_constructor_defaults_and_argument_checks():
    import inspect
    from neuralmonkey_amd import tf_shim
    from neuralmonkey_amd.decoders import Classifier, SequenceRegressor
    from neuralmonkey_amd.encoders import (AttentiveEncoder, SequenceAveragePooling, SequenceMaxPooling,
                                           SequencePooling)
    from neuralmonkey_amd.model.gradient_reversal import SpatialStatefulView, StatefulView, TemporalStatefulView
    from neuralmonkey_amd.model.sequence import EmbeddedSequence
    from neuralmonkey_amd.model.stateful import Stateful
    from neuralmonkey_amd.runners import LogitsRunner, RegressionRunner
    from neuralmonkey_amd.runtime import reset_registry
    defaults = {k: p.default for k, p in inspect.signature(Classifier.__init__).parameters.items()}
    assert defaults["dropout_keep_prob"] == 0.5 and defaults["activation_fn"] is tf_shim.nn.relu
    defaults = {k: p.default for k, p in inspect.signature(SequenceRegressor.__init__).parameters.items()}
    assert (defaults["layers"], defaults["dropout_keep_prob"], defaults["dimension"]) == (None, 1.0, 1)
    reset_registry()
    seq = EmbeddedSequence("seq", M.words(3), "source", 4)
    pool, avg = SequenceMaxPooling("pool", seq), SequenceAveragePooling("avg", seq)
    assert issubclass(SequenceMaxPooling, SequencePooling) and isinstance(pool, Stateful)
    assert pool.output_size == avg.output_size == 4 and pool.input_sequence is seq
    with pytest.raises(TypeError):
        SequenceMaxPooling("pool2", "seq")
    att = AttentiveEncoder("att", seq, hidden_size=5, num_heads=3)
    assert (att.dimension, att.output_size) == (4, 12)
    att2 = AttentiveEncoder("att2", seq, hidden_size=5, num_heads=3, output_size=7, state_proj_size=2)
    assert (att2.dimension, att2.output_size) == (2, 7)
    for keep in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError, match=r"Dropout keep prob must be inside \(0,1\]"):
            AttentiveEncoder("att3", seq, hidden_size=5, num_heads=3, dropout_keep_prob=keep)
    with pytest.raises(TypeError):
        AttentiveEncoder("att4", seq, hidden_size="5", num_heads=3)
    view = StatefulView(pool)
    assert view.output_size == 4 and view.output.key == pool.output.key
    assert "_reversed_object" in view.dependencies and pool in view.get_dependencies()[0]
    tview = TemporalStatefulView(att)
    assert tview.dimension == att.dimension and tview.temporal_states.key == att.temporal_states.key
    assert tview.temporal_mask.key == att.temporal_mask.key
    with pytest.raises(TypeError):
        StatefulView(seq)                                         # a sequence has no ``output``
    with pytest.raises(TypeError):
        SpatialStatefulView(att)
    cls = Classifier("cls", [pool, att], M.words(5), "target", [6])
    assert cls.input_dimension == 16 and cls.decoded.key == cls.decoded_seq.key == cls.decoded_symbols.key
    with pytest.raises(TypeError):
        Classifier("cls2", pool, M.words(5), "target", [6])      # encoders is a list
    with pytest.raises(TypeError):
        Classifier("cls3", [pool], M.words(5), "target")         # ``layers`` has no default
    with pytest.raises(NotImplementedError, match="activation"):
        Classifier("cls4", [pool], M.words(5), "target", [3], activation_fn=len)
    reg = SequenceRegressor("reg", [view], "count", dimension=2)
    assert reg.layer_sizes == [] and reg.input_dimension == 4 and reg.decoded.key == reg.predictions.key
    with pytest.raises(ValueError, match="Either a pick index or a vocabulary value"):
        LogitsRunner("dist", cls, pick_index=1, pick_value="w1")
    with pytest.raises(ValueError, match="Value 'nope' is not in vocabulary of decoder 'cls'"):
        LogitsRunner("dist", cls, pick_value="nope")
    assert LogitsRunner("dist", cls, pick_value="w1").pick_index == cls.vocabulary.index_to_word.index("w1")
    with pytest.raises(TypeError):
        RegressionRunner("count", reg, postprocess="no")
    assert RegressionRunner("count", reg).decoder_data_id == "count"


def test_max_pooling_refuses_a_batch_without_tokens_on_the_fed_arrays():
    """The reference's tf.assert_greater(sum(mask), 0.5) -- checked in stage_inputs, on the host, so that a captured
    step makes it too; average pooling has no such assertion."""
    from neuralmonkey_amd.encoders import SequenceAveragePooling, SequenceMaxPooling
    from neuralmonkey_amd.encoders.numpy_stateful_filler import TemporalFiller
    from neuralmonkey_amd.runtime import reset_registry
    reset_registry()
    filler = TemporalFiller("states", "features", 3)
    pool, avg = SequenceMaxPooling("pool", filler), SequenceAveragePooling("avg", filler)

    class Ctx:
        def __init__(self, lengths):
            self.feed = {filler.states_input: np.zeros((len(lengths), 4, 3), np.float32),
                         filler.lengths_input: np.asarray(lengths, np.int32)}

        def is_fed(self, p):
            return p in self.feed

        def fed(self, p):
            return self.feed[p]
    pool.stage_inputs(Ctx([0, 2]))
    avg.stage_inputs(Ctx([0, 0]))
    with pytest.raises(ValueError, match="holds no token"):
        pool.stage_inputs(Ctx([0, 0]))


# ---- the order of the deferred backward passes -----------------------------------------------------------------------------
def test_deferred_backward_passes_run_once_after_everything_that_reads_them():
    """A pooler and an attentive encoder read one recurrent encoder; a second decoder reads the pooler again through a
    view.  Whatever order the gradients arrive in, every part runs once, on the sum, after its readers."""
    from neuralmonkey_amd.runtime import RunContext, part_reads

    def send(ctx, target):
        """One gradient per target (a second one would be summed on the device)."""
        slot = ctx.memo.get("pending_backward", {}).get(target)
        ctx.defer_backward(target, "gradient" if slot is None or slot[0] is None else None, None)

    class Part:
        def __init__(self, name, log, **reads):
            self.name, self.log = name, log
            for k, v in reads.items():
                setattr(self, k, v)

        def backward(self, ctx, d_states, d_final):
            self.log.append(self.name)
            for attr in ("input_sequence", "_reversed_object", "input_for_cross_attention"):
                if getattr(self, attr, None) is not None:
                    send(ctx, getattr(self, attr))

    class Seq(Part):
        def backward(self, ctx, d_states, d_final=None):            # a sequence has no final output
            assert d_states == "gradient" and d_final is None
            self.log.append(self.name)

    import itertools
    for order in itertools.permutations(["att", "pool", "view", "other"]):
        log = []
        seq = Seq("seq", log)
        rnn = Part("rnn", log, input_sequence=seq)
        other = Part("other", log, input_sequence=seq, input_for_cross_attention=rnn)
        parts = {"att": Part("att", log, input_sequence=rnn), "pool": Part("pool", log, input_sequence=rnn),
                 "other": other}
        parts["view"] = Part("view", log, _reversed_object=parts["pool"])
        assert part_reads(parts["view"]) == [parts["pool"]] and part_reads(other) == [seq, rnn]
        ctx = RunContext(None, {})
        ctx.memo["backward_deferred"] = True
        for name in order:
            send(ctx, parts[name])
        ctx.flush_backward()
        assert sorted(log) == ["att", "other", "pool", "rnn", "seq", "view"], log        # each exactly once
        pos = {n: i for i, n in enumerate(log)}
        assert pos["view"] < pos["pool"] < pos["rnn"] < pos["seq"] and pos["att"] < pos["rnn"]
        assert pos["other"] < pos["rnn"] and pos["other"] < pos["seq"]


# ---- the fourth binding table ---------------------------------------------------------------------------------------------
def pool_header_symbols():
    text = open(os.path.join(ROOT, "include", "nmhip_pool.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nm_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


def test_pool_header_matches_its_binding_table(lib):
    from neuralmonkey_amd import _lib
    from .test_abi import header_symbols
    from .test_ctc_host import ctc_header_symbols
    from .test_labeler_host import label_header_symbols
    mine = pool_header_symbols()
    assert mine == set(_lib.POOL_SIGNATURES) and len(mine) == 5
    for other in (_lib.SIGNATURES, _lib.CTC_SIGNATURES, _lib.LABEL_SIGNATURES):
        assert not mine & set(other)
    assert not mine & header_symbols() and not mine & ctc_header_symbols() and not mine & label_header_symbols()
    for name, (res, args) in _lib.POOL_SIGNATURES.items():
        fn = getattr(lib, name)                                          # exported, and bound by load()
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_pool_entry_points_refuse_before_any_launch(lib):
    """Host buffers and a null stream: a call that got as far as a launch would fault or fail differently."""
    buf = (ctypes.c_float * 4096)()
    other = (ctypes.c_float * 4096)()
    ibuf = (ctypes.c_int32 * 4096)()

    def fwd(mode=0, x=buf, ldx=8, mask=buf, b=2, t=3, d=8, out=other, ldo=8, ties=ibuf):
        return lib.nm_pool_fwd(None, mode, x, ldx, mask, b, t, d, out, ldo, ties)
    for kwargs, text in ((dict(mode=2), b"nm_pool_fwd: mode 2 is neither NM_POOL_MAX nor NM_POOL_AVG"),
                         (dict(b=0), b"nm_pool_fwd: bad sizes B 0, T 3, D 8"),
                         (dict(t=0), b"nm_pool_fwd: bad sizes"), (dict(d=0), b"nm_pool_fwd: bad sizes"),
                         (dict(b=1 << 20, t=1 << 12), b"nm_pool_fwd: B*T = 4294967296 rows beyond 2^31"),
                         (dict(ldx=7), b"nm_pool_fwd: ldx 7 below D 8"), (dict(ldo=7), b"nm_pool_fwd: ldo 7 below D 8"),
                         (dict(x=None), b"nm_pool_fwd: null pointer"), (dict(mask=None), b"nm_pool_fwd: null pointer"),
                         (dict(out=None), b"nm_pool_fwd: null pointer"),
                         (dict(ties=None), b"nm_pool_fwd: NM_POOL_MAX without ties")):
        assert fwd(**kwargs) < 0 and text in lib.nm_last_error(), (kwargs, lib.nm_last_error())

    def bwd(mode=0, x=buf, ldx=8, mask=buf, out=other, ldo=8, ties=ibuf, dout=other, lddo=8, b=2, t=3, d=8, dx=None,
            lddx=8, acc=0):
        dx = ctypes.byref(other, 4 * 1024) if dx is None else dx
        return lib.nm_pool_bwd(None, mode, x, ldx, mask, out, ldo, ties, dout, lddo, b, t, d, dx, lddx, acc)
    for kwargs, text in ((dict(mode=-1), b"nm_pool_bwd: mode -1"), (dict(d=0), b"nm_pool_bwd: bad sizes"),
                         (dict(lddo=7), b"nm_pool_bwd: lddo 7 below D 8"), (dict(lddx=7), b"nm_pool_bwd: lddx 7 below"),
                         (dict(ldx=7), b"nm_pool_bwd: ldx 7 below D 8"), (dict(ldo=7), b"nm_pool_bwd: ldo 7 below D 8"),
                         (dict(dout=None), b"nm_pool_bwd: null pointer"), (dict(mode=1, mask=None), b"null pointer"),
                         (dict(x=None), b"nm_pool_bwd: NM_POOL_MAX without x, out or ties"),
                         (dict(ties=None), b"nm_pool_bwd: NM_POOL_MAX without x, out or ties"),
                         (dict(dx=buf), b"nm_pool_bwd: dx aliasing x"),
                         (dict(dx=ctypes.byref(buf, 4 * 40)), b"nm_pool_bwd: dx aliasing x")):
        assert bwd(**kwargs) < 0 and text in lib.nm_last_error(), (kwargs, lib.nm_last_error())

    def sm(e=buf, lde=4, mask=buf, b=2, t=3, h=4, w=other, ldw=4, s=other, lds=4, z=other):
        return lib.nm_time_softmax_fwd(None, e, lde, mask, b, t, h, w, ldw, s, lds, z)
    for kwargs, text in ((dict(h=0), b"nm_time_softmax_fwd: bad sizes B 2, T 3, H 0"), (dict(t=0), b"bad sizes"),
                         (dict(lde=3), b"nm_time_softmax_fwd: lde 3 below H 4"),
                         (dict(ldw=3), b"nm_time_softmax_fwd: ldw 3 below H 4"),
                         (dict(lds=3), b"nm_time_softmax_fwd: lds 3 below H 4"),
                         (dict(e=None), b"nm_time_softmax_fwd: null pointer"),
                         (dict(w=None), b"nm_time_softmax_fwd: null pointer"),
                         (dict(b=1 << 20, t=1 << 12), b"beyond the grid")):
        assert sm(**kwargs) < 0 and text in lib.nm_last_error(), (kwargs, lib.nm_last_error())

    def smb(dw=buf, lddw=4, s=other, lds=4, z=other, mask=buf, b=2, t=3, h=4, de=None, ldde=4, acc=0):
        de = ctypes.byref(other, 4 * 1024) if de is None else de
        return lib.nm_time_softmax_bwd(None, dw, lddw, s, lds, z, mask, b, t, h, de, ldde, acc)
    for kwargs, text in ((dict(b=0), b"nm_time_softmax_bwd: bad sizes"), (dict(lddw=3), b"lddw 3 below H 4"),
                         (dict(lds=3), b"lds 3 below H 4"), (dict(ldde=3), b"ldde 3 below H 4"),
                         (dict(s=None), b"nm_time_softmax_bwd: null pointer"),
                         (dict(z=None), b"nm_time_softmax_bwd: mask without z"),
                         (dict(de=buf, acc=1), b"nm_time_softmax_bwd: accumulate into dw itself")):
        assert smb(**kwargs) < 0 and text in lib.nm_last_error(), (kwargs, lib.nm_last_error())

    def sq(pred=buf, ld=2, rows=3, dim=2, y=other, loss=other):
        return lib.nm_sqerr_rows(None, pred, ld, rows, dim, y, None, 1, loss)
    for kwargs, text in ((dict(dim=0), b"nm_sqerr_rows: dimension 0"), (dict(rows=-1), b"nm_sqerr_rows: bad row count"),
                         (dict(ld=1), b"nm_sqerr_rows: ld 1 below the dimension 2"),
                         (dict(pred=None), b"nm_sqerr_rows: null pointer"), (dict(y=None), b"nm_sqerr_rows: null pointer")):
        assert sq(**kwargs) < 0 and text in lib.nm_last_error(), (kwargs, lib.nm_last_error())
    assert sq(rows=0, pred=None, y=None) == 0                       # rows == 0 is a no-op


def test_kernels_of_the_pool_file_do_not_spill(lib):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_resources
    finally:
        sys.path.pop(0)
    mine = {k: v for k, v in kernel_resources().items()
            if any(s in k for s in ("pool_fwd_kernel", "pool_bwd_kernel", "time_softmax_", "sqerr_rows_kernel"))}
    assert len(mine) == 4 + 4 + 7 + 7 + 1, sorted(mine)
    assert all(v["scratch"] == 0 for v in mine.values())


# ---- the restatement against the reference's own numbers -------------------------------------------------------------------
def close(got, want, what, tol=1e-6):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(np.abs(want).max()), 1e-6)
    err = float(np.abs(got - want).max())
    assert err <= tol * scale, "{}: max |diff| {:.3e} (scale {:.3g})".format(what, err, scale)


def restate(z, cfg, params, dtype=np.float64, with_grads=False):
    """Every tensor of the fixture from the encoder's states on."""
    states, mask = z["out/enc_states"], z["out/enc_mask"]
    out, outputs, saved = {}, [], {}
    for kind in cfg["encoders"]:
        if kind == "max":
            out["max_output"] = R.max_pool(states, mask, dtype)["out"]
        elif kind == "avg":
            out["avg_output"] = R.avg_pool(states, mask, dtype)["out"]
        else:
            att = saved["att"] = R.attentive(params, states, mask, "encoder_att", dtype)
            out.update(att_output=att["output"], att_weights=att["attention_weights"],
                       att_temporal_states=att["temporal_states"],
                       att_temporal_mask=np.ones(att["temporal_states"].shape[:2], dtype))
        outputs.append(out[kind + "_output"])
    layers = len(cfg["layers"])
    if cfg["head"] == "classifier":
        head = R.classifier(params, outputs, z["in/tgt_ids"], "classifier", layers, cfg["activation"], dtype)
        out.update(decoded_seq=head["decoded"][None], decoded_logits=head["logits"][None],
                   runtime_logprobs=head["logprobs"][None], cost=head["cost"])
    elif cfg["head"] == "regressor":
        head = R.regressor(params, outputs, z["in/targets"], "regressor", layers, cfg["activation"], dtype)
        out.update(predictions=head["predictions"], cost=head["cost"])
    return out


def test_fixture_directory_holds_the_issues_cases():
    have = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(M.FIX, "*.npz")))
    assert have == sorted(M.FORWARD_CASES)
    for case in M.FORWARD_CASES:
        z, cfg, _ = M.load_fixture(case)
        lengths = z["out/enc_mask"].sum(axis=1).astype(int).tolist()
        assert len(lengths) == 5 and 1 in lengths and len(set(lengths)) >= 3 and max(lengths) == 7     # ragged
        assert any("never-seen" in [str(t) for t in row] for row in z["in/src_tokens"])
        assert os.path.getsize(os.path.join(M.FIX, case + ".npz")) < 64 * 1024
    for case in M.FD_CASES:
        z, cfg, params = M.load_fixture(case)
        assert cfg["activation"] == "tanh" and "max" in cfg["encoders"]
        names = [str(n) for n in z["fd/names"]]
        assert set(names) == set(params)                              # no variable left out
        assert all(names.count(n) == min(4, params[n].size) for n in params)


@pytest.mark.parametrize("case", M.FORWARD_CASES)
def test_restatement_reproduces_the_reference(case):
    z, cfg, params = M.load_fixture(case)
    got = restate(z, cfg, params)
    keys = [k[4:] for k in z.files if k.startswith("out/") and k[4:] in got]
    assert len(keys) >= 1 + (3 if "att" in cfg["encoders"] else 0) + (2 if cfg["head"] else 0)
    for key in keys:
        if key == "decoded_seq":
            assert np.array_equal(got[key], z["out/" + key])
        else:
            close(got[key], z["out/" + key], case + " " + key)
    if cfg["head"] == "classifier":
        words = ["<pad>", "<s>", "</s>", "<unk>"] + ["w{}".format(i) for i in range(cfg["cls_vocab"])]
        assert [words[i] for i in got["decoded_seq"][0]] == [str(s) for s in z["out/runner_greedy"]]
        for tag, kw in (("logits", {}), ("logits_raw_pick0", dict(normalize=False, pick_index=0)),
                        ("logits_pick", dict(pick_index=words.index("w2")))):
            mine = R.parse_logits_strings(R.logits_runner_strings(z["out/decoded_logits"], **kw))
            theirs = R.parse_logits_strings([[str(s)] for s in z["out/runner_" + tag]])
            close(mine, theirs, case + " runner " + tag, 1e-6)
        assert R.parse_logits_strings([[str(s)] for s in z["out/runner_logits_raw_pick0"]]).shape == (
            5, len(words))                                            # index 0 is "all classes"
        assert R.parse_logits_strings([[str(s)] for s in z["out/runner_logits_pick"]]).shape == (5, 1)
    if cfg["head"] == "regressor":
        close(z["out/runner_predictions"], got["predictions"], case + " runner predictions")
        close(z["out/runner_mse"], got["cost"], case + " runner mse")


# ---- the restatement's analytic gradients against torch float64 autograd --------------------------------------------------
def _t(a, grad=True):
    import torch
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def torch_max_pool(x, m):
    """tf.reduce_max's gradient splits evenly among equal maxima: torch.amax does the same."""
    import torch
    return torch.amax(x * m[:, :, None] + 1e-15 * (1 - m[:, :, None]), dim=1)


def torch_time_softmax(e, m):
    import torch
    s = torch.softmax(e, dim=1)
    if m is None:
        return s
    u = s * m[:, :, None]
    return u / (u.sum(dim=1, keepdim=True) + 1e-8)


def torch_attentive(p, x, m, name):
    import torch
    bsz, steps, d = x.shape
    flat = x.reshape(-1, d)
    energies = (torch.tanh(flat @ p[name + "/S1/kernel"]) @ p[name + "/S2/kernel"]).reshape(bsz, steps, -1)
    w = torch_time_softmax(energies, m)
    proj = x
    if name + "/state_projection/kernel" in p:
        proj = (flat @ p[name + "/state_projection/kernel"] + p[name + "/state_projection/bias"]).reshape(bsz, steps, -1)
    out = torch.einsum("bth,btd->bhd", w, proj).reshape(bsz, -1)
    if name + "/output_projection/kernel" in p:
        out = out @ p[name + "/output_projection/kernel"] + p[name + "/output_projection/bias"]
    return out


def torch_mlp(p, x, prefix, layers, activation):
    import torch
    act = {"relu": torch.relu, "tanh": torch.tanh}[activation]
    for i in range(layers):
        x = act(x @ p["{}/mlp_layer_{}/kernel".format(prefix, i)] + p["{}/mlp_layer_{}/bias".format(prefix, i)])
    return x


def torch_classifier_cost(p, x, targets, name, layers, activation):
    import torch
    hidden = torch_mlp(p, x, name + "/multilayer_perceptron/deep_output_mlp", layers, activation)
    top = name + "/multilayer_perceptron/classification_layer/"
    logits = hidden @ p[top + "kernel"] + p[top + "bias"]
    return torch.nn.functional.cross_entropy(logits, torch.tensor(np.asarray(targets), dtype=torch.long))


def test_kernel_level_gradients_equal_float64_autograd():
    import torch
    rng = np.random.default_rng(7)
    lengths = [7, 1, 3, 0, 7]
    mask = (np.arange(7)[None, :] < np.asarray(lengths)[:, None]).astype(np.float64)
    x = rng.standard_normal((5, 7, 6))
    x[0, 2, 0] = x[0, 5, 0] = 7.25                                  # a tie: half the gradient each
    x[2, :, 1] = -np.abs(x[2, :, 1]) - 0.5                          # negative everywhere, padded: pools to 1e-15
    dout = rng.standard_normal((5, 6))
    xt, mt = _t(x), _t(mask, False)
    torch_max_pool(xt, mt).backward(_t(dout, False))
    mine = R.max_pool_bwd(x, mask, dout)
    assert np.abs(mine - xt.grad.numpy()).max() <= 1e-12 and mine[0, 2, 0] == mine[0, 5, 0] == dout[0, 0] / 2
    assert R.max_pool(x, mask)["out"][2, 1] == 1e-15 and not mine[2, :, 1].any()
    xt = _t(x)
    ((xt * mt[:, :, None]).sum(dim=1) / (mt.sum(dim=1, keepdim=True) + 1e-8)).backward(_t(dout, False))
    assert np.abs(R.avg_pool_bwd(mask, dout, 6) - xt.grad.numpy()).max() <= 1e-12
    assert not R.avg_pool(x, mask)["out"][3].any()                   # length 0: exact zeros
    e = 2.0 * rng.standard_normal((5, 7, 3))
    e[0] += 100.0
    e[2] -= 110.0
    dw = rng.standard_normal((5, 7, 3))
    for m in (mask, None):
        et = _t(e)
        torch_time_softmax(et, None if m is None else mt).backward(_t(dw, False))
        f = R.time_softmax(e, m)
        mine = R.time_softmax_bwd(dw, f["s"], f["z"], m)
        assert np.abs(mine - et.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(et.grad.numpy()).max())
    p, y = rng.standard_normal((5, 2)), rng.standard_normal(5)
    pt = _t(p)
    (0.37 * ((pt - _t(y, False)[:, None]) ** 2).sum()).backward()
    assert np.abs(R.sqerr(p, y, 0.37)["grad"] - pt.grad.numpy()).max() <= 1e-12


@pytest.mark.parametrize("case", M.FD_CASES + ["classifier_attentive_maxpool", "regressor_two_dimensions"])
def test_model_gradients_of_the_restatement_equal_float64_autograd_and_the_references_differences(case):
    """From the encoder's states on: every head / pooling-encoder variable's gradient and d states to 1e-12; on the FD
    fixtures those variables' gradients also agree with the reference's central differences."""
    import torch
    z, cfg, params = M.load_fixture(case)
    states, mask = z["out/enc_states"], z["out/enc_mask"]
    names = [n for n in params if n.split("/")[0] in ("encoder_att", "classifier", "regressor")]
    p = {n: _t(params[n]) for n in names}
    xt, mt = _t(states), _t(mask, False)
    outputs = []
    for kind in cfg["encoders"]:
        if kind == "max":
            outputs.append(torch_max_pool(xt, mt))
        elif kind == "avg":
            outputs.append((xt * mt[:, :, None]).sum(dim=1) / (mt.sum(dim=1, keepdim=True) + 1e-8))
        else:
            outputs.append(torch_attentive(p, xt, mt, "encoder_att"))
    cat = torch.cat(outputs, dim=1)
    layers = len(cfg["layers"])
    if cfg["head"] == "classifier":
        cost = torch_classifier_cost(p, cat, z["in/tgt_ids"], "classifier", layers, cfg["activation"])
    else:
        hidden = torch_mlp(p, cat, "regressor/mlp", layers, cfg["activation"])
        pred = hidden @ p["regressor/output_projection/kernel"] + p["regressor/output_projection/bias"]
        cost = ((pred - _t(z["in/targets"], False)[:, None]) ** 2).mean()
    cost.backward()
    # the restatement, composed the same way
    mine, d_states = {}, np.zeros(states.shape)
    got = restate(z, cfg, params)
    assert abs(float(got["cost"]) - float(cost.detach())) <= 1e-12
    outs = [got[k + "_output"] for k in cfg["encoders"]]
    if cfg["head"] == "classifier":
        head = R.classifier(params, outs, z["in/tgt_ids"], "classifier", layers, cfg["activation"])
    else:
        head = R.regressor(params, outs, z["in/targets"], "regressor", layers, cfg["activation"])
    mine.update(head["grads"])
    d_in, col = mine.pop("inputs"), 0
    for kind, o in zip(cfg["encoders"], outs):
        d_out = d_in[:, col:col + o.shape[1]]
        col += o.shape[1]
        if kind == "max":
            d_states += R.max_pool_bwd(states, mask, d_out)
        elif kind == "avg":
            d_states += R.avg_pool_bwd(mask, d_out, states.shape[2])
        else:
            g, dx = R.attentive_bwd(R.attentive(params, states, mask), d_output=d_out)
            mine.update(g)
            d_states += dx
    assert set(mine) == set(names)
    for n in names:
        assert np.abs(mine[n] - p[n].grad.numpy()).max() <= 1e-12, n
    assert np.abs(d_states - xt.grad.numpy()).max() <= 1e-12
    if case in M.FD_CASES:
        for name, i, fd in zip([str(n) for n in z["fd/names"]], z["fd/index"], z["fd/value"]):
            if name in mine:
                g = float(mine[name].reshape(-1)[int(i)])
                assert abs(g - fd) <= 6e-3 + 2e-2 * abs(fd), (name, i, g, fd)


def test_adversarial_topology_restatement_equals_float64_autograd():
    """relu, two decoders, one through a gradient-reversal view: the adversary's own variables get the plain gradient
    of its cost, everything behind the view the negated one."""
    import torch

    class Reverse(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.view_as(x)

        @staticmethod
        def backward(ctx, grad):
            return -grad
    cfg = M.TOPOLOGY
    states, targets = M.topology_data()
    steps = max(cfg["lengths"])
    x = np.zeros((len(states), steps, cfg["dim"]))
    for i, s in enumerate(states):
        x[i, :len(s)] = s
    mask = (np.arange(steps)[None, :] < np.asarray(cfg["lengths"])[:, None]).astype(np.float64)
    ids = np.asarray([3 if t[0] == "never-seen" else 4 + int(t[0][1:]) for t in targets])
    rng = np.random.default_rng(3)
    shapes = {"encoder_att/S1/kernel": (6, 7), "encoder_att/S2/kernel": (7, 3),
              "encoder_att/state_projection/kernel": (6, 4), "encoder_att/state_projection/bias": (4,),
              "encoder_att/output_projection/kernel": (12, 9), "encoder_att/output_projection/bias": (9,),
              "classifier/multilayer_perceptron/deep_output_mlp/mlp_layer_0/kernel": (15, 8),
              "classifier/multilayer_perceptron/deep_output_mlp/mlp_layer_0/bias": (8,),
              "classifier/multilayer_perceptron/classification_layer/kernel": (8, 10),
              "classifier/multilayer_perceptron/classification_layer/bias": (10,),
              "classifier_adv/multilayer_perceptron/classification_layer/kernel": (6, 10),
              "classifier_adv/multilayer_perceptron/classification_layer/bias": (10,)}
    params = {n: 0.4 * rng.standard_normal(s) for n, s in shapes.items()}
    p = {n: _t(v) for n, v in params.items()}
    xt, mt = _t(x), _t(mask, False)
    pooled = torch_max_pool(xt, mt)
    main = torch_classifier_cost(p, torch.cat([torch_attentive(p, xt, mt, "encoder_att"), pooled], dim=1), ids,
                                 "classifier", 1, "relu")
    adv = torch_classifier_cost(p, Reverse.apply(pooled), ids, "classifier_adv", 0, "relu")
    (main + adv).backward()
    mine = R.adversarial_topology(params, x, mask, ids, 1, "relu")
    assert abs(float(mine["cost"]) - float((main + adv).detach())) <= 1e-12
    assert set(mine["grads"]) == set(params) | {"states"}
    for n in params:
        assert np.abs(mine["grads"][n] - p[n].grad.numpy()).max() <= 1e-12, n
    assert np.abs(mine["grads"]["states"] - xt.grad.numpy()).max() <= 1e-12
    tie = mine["grads"]["states"][0, [1, 4], 0]
    assert tie[0] != 0 and x[0, 1, 0] == x[0, 4, 0] == 3.5          # the two maxima of column 0 of sentence 0 ...
    pool_share = R.max_pool_bwd(x, mask, mine["d_pool"])[0, [1, 4], 0]
    assert pool_share[0] == pool_share[1] == mine["d_pool"][0, 0] / 2       # ... take half the pooler's gradient each


# ---- the runners' collection of results --------------------------------------------------------------------------------------
def test_runners_collect_results_as_the_reference_does():
    from neuralmonkey_amd.decoders import Classifier, SequenceRegressor
    from neuralmonkey_amd.encoders import SequenceMaxPooling
    from neuralmonkey_amd.model.sequence import EmbeddedSequence
    from neuralmonkey_amd.runners import LogitsRunner, RegressionRunner
    from neuralmonkey_amd.runtime import reset_registry
    reset_registry()
    seq = EmbeddedSequence("seq", M.words(3), "source", 4)
    pool = SequenceMaxPooling("pool", seq)
    cls = Classifier("cls", [pool], M.words(2), "target", [])
    logits = np.asarray([[[0.5, -1.0, 2.0, 0.25, 0.0, 1.0], [3.0, 3.0, -2.0, 0.0, 0.5, 0.125]]], np.float32)
    result = {"logits": logits, "train_loss": 0.5, "runtime_loss": 0.25}
    for kw in (dict(), dict(normalize=False), dict(pick_index=0), dict(pick_index=2), dict(normalize=False, pick_index=4)):
        runner = LogitsRunner("dist", cls, **kw)
        ex = runner.get_executable(compute_losses=True, summaries=False, num_sessions=1)
        fetches, _ = ex.next_to_execute()
        assert set(fetches) == {"logits", "train_loss", "runtime_loss"}
        ex.collect_results([result])
        want = R.logits_runner_strings(logits, kw.get("normalize", True), kw.get("pick_index"))
        assert ex.result.outputs["dist"] == want
        assert ex.result.losses == {"dist/train_loss": 0.5, "dist/runtime_loss": 0.25}
        values = R.parse_logits_strings(ex.result.outputs["dist"])
        assert values.shape == (2, 1 if kw.get("pick_index") else 6)           # index 0 is "all classes"
        if kw.get("normalize", True) and not kw.get("pick_index"):
            assert np.allclose(values.sum(axis=1), 1.0, atol=1e-6)
        with pytest.raises(ValueError, match="LogitsRunner needs exactly 1 execution result, got 2"):
            runner.get_executable(True, False, 2).collect_results([result, result])
    big = {"logits": np.asarray([[[1000.0, 0.0, 0.0, 0.0, 0.0, 0.0]]], np.float32), "train_loss": 0.0, "runtime_loss": 0.0}
    ex = LogitsRunner("dist", cls).get_executable(True, False, 1)
    with np.errstate(over="ignore", invalid="ignore"):
        ex.collect_results([big])
    assert ex.result.outputs["dist"][0][0].startswith("nan")        # no maximum subtracted: as the reference
    ex = LogitsRunner("dist", cls).get_executable(False, False, 1)
    assert ex.next_to_execute()[0]["train_loss"] == 0.0 and ex.next_to_execute()[0]["runtime_loss"] == 0.0

    reg = SequenceRegressor("reg", [pool], "count", dimension=2)
    runner = RegressionRunner("count", reg, postprocess=lambda rows: [[2 * v for v in r] for r in rows])
    ex = runner.get_executable(compute_losses=True, summaries=False, num_sessions=2)
    a = {"prediction": np.asarray([[1.0, 2.0], [3.0, 4.0]], np.float32), "mse": np.float32(0.5)}
    b = {"prediction": np.asarray([[3.0, 2.0], [5.0, 0.0]], np.float32), "mse": np.float32(0.25)}
    ex.collect_results([a, b])
    assert ex.result.outputs["count"] == [[4.0, 4.0], [8.0, 4.0]] and ex.result.losses == {"count/mse": 0.75}
    ex = RegressionRunner("count", reg).get_executable(compute_losses=False, summaries=False, num_sessions=1)
    assert ex.next_to_execute()[0]["mse"] == 0.0 and set(ex.next_to_execute()[0]) == {"prediction", "mse"}
