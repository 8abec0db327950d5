"""Supervised attention without a GPU: the reference's class paths and its configuration (tests/alignment.ini from the
committed archive) through the config loader, the preprocessor against a stored run of the reference's own, constructor
signatures, the refusals of the three engine decisions, and the binding table of include/nmhip_align.h
with its argument checks on the CPU-built library.

tests/alignment.ini AS IT IS cannot be built by the reference either: its decoder has ``embedding_size=9`` and
``maxout_size=7``, which decoders/decoder.py:337-342 of the reference refuses with a ValueError ("The dimension (7) of the
output projection must be same as the dimension of the input embedding (9)") -- the configuration is commented out in
the reference's tests/tests_run.sh:11.  This engine mirrors that refusal (decoders/decoder.py), so the verbatim file is
pinned to that error, and everything else is asserted on the file with that ONE value changed (``maxout_size=9``)."""
import ctypes
import json
import os
import re
import tarfile

import numpy as np
import pytest

from .test_reference_inis import BUNDLE as TEXT_BUNDLE, REF

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
BUNDLE = os.path.join(GOLDEN, "reference_tests_alignment.tar.gz")
LISTS = os.path.join(GOLDEN, "alignment_signatures.json")
PREPROCESSED = os.path.join(GOLDEN, "alignment_preprocessor.npz")


@pytest.fixture(scope="module")
def ref_root(tmp_path_factory):
    """tests/alignment.ini, tests/data/train.tc.ali and the text the configuration names: the two archives, extracted."""
    root = tmp_path_factory.mktemp("reference_tests_alignment")
    for bundle in (TEXT_BUNDLE, BUNDLE):
        with tarfile.open(bundle) as tar:
            tar.extractall(root)
    return str(root)


def with_matching_maxout(ref_root):
    """tests/alignment.ini with ``maxout_size=7`` -> ``maxout_size=9`` (the decoder's embedding size), nothing else."""
    text = open(os.path.join(ref_root, "tests", "alignment.ini")).read()
    edited, n = re.subn(r"^maxout_size=7$", "maxout_size=9", text, flags=re.M)
    assert n == 1 and "embedding_size=9" in text
    with open(os.path.join(ref_root, "tests", "alignment_maxout9.ini"), "w") as handle:
        handle.write(edited)
    return "alignment_maxout9"


# ---- through the config loader ------------------------------------------------------------------------------------------
def test_alignment_ini_builds(ref_root):
    """Fails on a tree without the feature: its classes are not there to import, and the loader answers the file with
    SymbolNotShipped."""
    from neuralmonkey_amd.attention import Attention
    from neuralmonkey_amd.config.builder import OutOfScope
    from neuralmonkey_amd.decoders import Decoder, WordAlignmentDecoder
    from neuralmonkey_amd.processors.alignment import WordAlignmentPreprocessor
    from neuralmonkey_amd.runners import GreedyRunner
    from neuralmonkey_amd.trainers import CrossEntropyTrainer
    from .test_reference_inis import load_verbatim
    model = load_verbatim(ref_root, with_matching_maxout(ref_root), device="cpu")
    trainer, = model.trainers
    assert isinstance(trainer, CrossEntropyTrainer) and isinstance(model.runners[0], GreedyRunner)
    dec, wad = [o.decoder for o in trainer.objectives]
    assert isinstance(dec, Decoder) and isinstance(wad, WordAlignmentDecoder) and wad.name == "alignment_decoder"
    assert [o.weight for o in trainer.objectives] == [1., 1e-3]
    assert [o.name for o in trainer.objectives] == ["bahdanau_decoder - cost", "alignment_decoder - cost"]
    assert wad.decoder is dec and wad.encoder is dec.encoders[0] and wad.data_id == "ali"
    assert isinstance(model.evaluation[0][-1], OutOfScope)              # evaluators.BLEUEvaluator stays a placeholder
    # no variables of its own
    store = model.tf_manager.sessions[0].store
    assert not [n for n in store.names() if n.startswith("alignment_decoder")]
    assert wad.variable_names(store) == []
    # Decoder.get_attention_object: the section's attention, whatever the mode
    att = dec.attentions[0]
    assert type(att) is Attention and att.name == "attention_sentence_encoder"          # pylint: disable=unidiomatic-typecheck
    assert dec.get_attention_object(wad.encoder, True) is att and dec.get_attention_object(wad.encoder, False) is att
    assert wad.attention is att
    # the fed alignment of the first batch
    assert wad.input_shapes == {"ali": [None, 8, 12]} and wad.input_types == {"ali": float}
    batch = next(iter(model.train_dataset.batches()))
    fd = wad.feed_dict(batch, train=True)
    ali = fd[wad.ref_alignment]
    assert ali.shape == (16, 8, 12) and ali.dtype == np.float32
    sums = ali.sum(axis=2)
    assert np.all((np.abs(sums - 1.0) < 1e-6) | (sums == 0.0)) and (sums == 0.0).any() and (sums > 0.5).any()
    pre = WordAlignmentPreprocessor(source_len=12, target_len=8)
    for row, tokens in zip(ali, batch.get_series("aligiza")):
        assert np.array_equal(row, pre(list(tokens)))
    # flags the trainer reads
    assert wad.loss_is_batch_sum is True and wad.cost.key == wad.train_loss.key
    assert wad.graph_safe_training(True) == dec.graph_safe_training(True)
    assert dec.uses_general_path(True)                                   # dropout_keep_prob=0.5: the taped path
    ctx = type("Ctx", (), {"fed": lambda self, p: dec.feed_dict(batch, train=True)[p]})()
    assert wad.train_token_count(ctx) == dec.train_token_count(ctx)
    assert wad in trainer.feedables and dec in wad.get_dependencies()[0]


def test_alignment_ini_as_it_is_is_refused_as_the_reference_refuses_it(ref_root):
    from .test_reference_inis import load_verbatim
    with pytest.raises(Exception) as info:
        load_verbatim(ref_root, "alignment", device="cpu")
    assert ("The dimension (7) of the output projection must be same as the dimension of the input embedding (9)"
            in str(info.value))


def test_archive_members_are_the_references_bytes(ref_root):
    with tarfile.open(BUNDLE) as tar:
        names = [m.name for m in tar.getmembers()]
    assert set(names) == {"tests/alignment.ini", "tests/data/train.tc.ali"}
    assert os.path.getsize(BUNDLE) < 16 * 1024
    if os.path.isdir(REF):
        for rel in names:
            with open(os.path.join(REF, rel), "rb") as a, open(os.path.join(ref_root, rel), "rb") as b:
                assert a.read() == b.read(), rel


# ---- the preprocessor against a stored run of the reference's ---------------------------------------------------------------
def test_preprocessor_reproduces_the_stored_run_of_the_reference(ref_root):
    from neuralmonkey_amd.processors.alignment import WordAlignmentPreprocessor
    z = np.load(PREPROCESSED)
    assert os.path.getsize(PREPROCESSED) < 16 * 1024
    with open(os.path.join(ref_root, "tests", "data", "train.tc.ali"), encoding="utf-8") as handle:
        lines = [line.rstrip("\n") for _, line in zip(range(32), handle)]
    assert lines == [str(s) for s in z["ini/lines"]] and z["ini/out"].shape == (32, 8, 12)
    pre = WordAlignmentPreprocessor(source_len=12, target_len=8)
    for line, want in zip(lines, z["ini/out"]):
        got = pre(line.split())
        assert got.dtype == want.dtype == np.float32 and np.array_equal(got, want)
    cases = sorted(k[:-5] for k in z.files if k.endswith("/args"))
    assert cases == ["colon_and_dash", "not_normalized", "not_normalized_float64", "one_based",
                     "one_based_out_of_range", "out_of_range", "weights"]
    seen = ""
    for name in cases:
        kwargs = json.loads(str(z[name + "/args"]))
        if "dtype" in kwargs:
            kwargs["dtype"] = getattr(np, kwargs["dtype"])
        pre = WordAlignmentPreprocessor(**kwargs)
        for line, want in zip(z[name + "/lines"], z[name + "/out"]):
            got = pre(str(line).split())
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (name, line)
            seen += " " + str(line)
    assert ":" in seen and "/0.5" in seen and "-" in seen
    assert z["not_normalized/out"].sum(axis=2).max() > 1.0 and z["out_of_range/out"].shape == (2, 2, 3)
    with pytest.raises(ValueError):
        WordAlignmentPreprocessor(3, 3)(["1-2-3"])                      # as the reference's two-name unpacking


# ---- signatures, refusals, flags ----------------------------------------------------------------------------------------
SIGNATURES = [("decoders/word_alignment_decoder.py", "WordAlignmentDecoder"),
              ("runners/word_alignment_runner.py", "WordAlignmentRunner"),
              ("processors/alignment.py", "WordAlignmentPreprocessor")]


@pytest.mark.parametrize("path,name", SIGNATURES)
def test_constructor_parameters_are_the_references(path, name):
    from .test_reference_signatures import product_parameters, read_reference_parameters
    with open(LISTS, encoding="utf-8") as handle:
        want = [tuple(p) for p in json.load(handle)[path][name]]
    if os.path.isdir(REF):
        assert read_reference_parameters(path, name) == want
    assert product_parameters(path, name) == want


def parts(second_encoder=False):
    from neuralmonkey_amd.encoders import SentenceEncoder
    from neuralmonkey_amd.runtime import reset_registry
    from neuralmonkey_amd.synthetic import synthetic_vocabulary
    reset_registry()
    vocab = synthetic_vocabulary(20)
    enc = SentenceEncoder(name="encoder", vocabulary=vocab, data_id="source", embedding_size=8, rnn_size=8,
                          max_input_len=7)
    other = SentenceEncoder(name="other", vocabulary=vocab, data_id="source", embedding_size=8, rnn_size=8,
                            max_input_len=7) if second_encoder else None
    return vocab, enc, other


def decoder_over(vocab, enc, attentions, rnn_size=8):
    from neuralmonkey_amd.decoders import Decoder
    return Decoder(encoders=[enc], vocabulary=vocab, data_id="target", name="decoder", max_output_len=5,
                   embedding_size=rnn_size, rnn_size=rnn_size, attentions=attentions)


def test_constructor_refusals_and_flags():
    from neuralmonkey_amd.attention import Attention, CoverageAttention, ScaledDotProdAttention
    from neuralmonkey_amd.decoders import WordAlignmentDecoder
    from neuralmonkey_amd.runners import WordAlignmentRunner
    vocab, enc, other = parts(second_encoder=True)
    att = Attention(name="attention", encoder=enc)
    dec = decoder_over(vocab, enc, [att])
    wad = WordAlignmentDecoder(enc, dec, "ali", "aligner")
    assert wad.attention is att and wad.loss_is_batch_sum is True and wad.input_shapes == {"ali": [None, 5, 7]}
    assert "decoder" in wad.dependencies and wad.enc_input is enc.input_sequence
    assert dec.get_attention_object(enc, True) is att and dec.get_attention_object(enc, False) is att
    # no attention over the encoder
    with pytest.raises(ValueError, match="Decoder 'decoder' has no attentions over the encoder 'other'"):
        dec.get_attention_object(other, True)
    with pytest.raises(ValueError, match="Decoder 'decoder' has no attentions over the encoder 'other'"):
        WordAlignmentDecoder(other, dec, "ali", "aligner2")
    with pytest.raises(TypeError):
        WordAlignmentDecoder(enc, att, "ali", "aligner3")                # ``decoder`` is a Decoder
    # the runner's KeyError, with the reference's text, for an attention the decoder never queries
    stray = Attention(name="stray", encoder=other)
    stray.bind_query_size(8)
    runner = WordAlignmentRunner("alignment", stray, dec)
    with pytest.raises(KeyError) as info:
        runner.fetches                                                   # pylint: disable=pointless-statement
    assert info.value.args[0] == "Attention has no recorded histories under key 'decoder_run'"
    good = WordAlignmentRunner("alignment", att, dec)
    assert set(good.fetches) == {"alignment"} and good.loss_names == [] and good.decoder is att
    assert dec in good.feedables and enc in good.feedables
    ex = good.get_executable(compute_losses=True, summaries=False, num_sessions=2)
    first, second = np.zeros((2, 7, 3), np.float32), np.ones((2, 7, 3), np.float32)
    ex.collect_results([{"alignment": first}, {"alignment": second}])
    assert ex.result.outputs["alignment"] is first and ex.result.losses == {}     # only the first session's result
    # two attentions over the encoder
    vocab, enc, _ = parts()
    dec2 = decoder_over(vocab, enc, [Attention(name="a1", encoder=enc), Attention(name="a2", encoder=enc)])
    with pytest.raises(ValueError, match="Decoder 'decoder' has 2 attentions over the encoder 'encoder'"):
        WordAlignmentDecoder(enc, dec2, "ali", "aligner")
    # attentions that do not record [T, B, S] weights of a feed-forward attention
    for make in (lambda e: CoverageAttention(name="cov", encoder=e),):
        vocab, enc, _ = parts()
        dec3 = decoder_over(vocab, enc, [make(enc)])
        with pytest.raises(TypeError, match="only attention.feed_forward.Attention"):
            WordAlignmentDecoder(enc, dec3, "ali", "aligner")
    vocab, enc, _ = parts()
    sdp = ScaledDotProdAttention(name="sdp", keys_encoder=enc)
    sdp.encoder = enc                                                    # (even if it named its encoder that way)
    dec4 = decoder_over(vocab, enc, [sdp], rnn_size=16)          # (queries as wide as the keys)
    with pytest.raises(TypeError, match="only attention.feed_forward.Attention"):
        WordAlignmentDecoder(enc, dec4, "ali", "aligner")


def test_fed_alignment_of_another_shape_is_refused_and_a_missing_series_feeds_zeros():
    from neuralmonkey_amd.attention import Attention
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    from neuralmonkey_amd.decoders import WordAlignmentDecoder
    vocab, enc, _ = parts()
    dec = decoder_over(vocab, enc, [Attention(name="attention", encoder=enc)])
    wad = WordAlignmentDecoder(enc, dec, "ali", "aligner")

    class Ctx:
        def __init__(self, feed):
            self.feed, self.memo = feed, {}

        def is_fed(self, p):
            return p in self.feed

        def fed(self, p):
            return self.feed[p]
    for shape in ((3, 5, 6), (3, 4, 7), (2, 5, 7), (3, 5, 7, 1), (3, 35)):
        ctx = Ctx({wad.ref_alignment: np.zeros(shape, np.float32), wad.batch_size: 3})
        with pytest.raises(ValueError, match=r"\[batch, max_output_len, max_length\] = \(3, 5, 7\) is expected"):
            wad.stage_inputs(ctx)
    series = {"source": [["w4"], ["w5", "w6"]], "ali": [np.eye(5, 7, dtype=np.float32), np.zeros((5, 7), np.float32)]}
    ds = Dataset("d", series, BatchingScheme(batch_size=2))
    fd = wad.feed_dict(ds, train=True)
    assert fd[wad.ref_alignment].shape == (2, 5, 7) and fd[wad.ref_alignment].dtype == np.float32
    assert np.array_equal(fd[wad.ref_alignment][0], np.eye(5, 7)) and fd[wad.train_mode] is True
    ds = Dataset("d", {"source": series["source"]}, BatchingScheme(batch_size=2))
    with pytest.warns(UserWarning, match="Training alignment not present!"):
        fd = wad.feed_dict(ds, train=True)
    assert fd[wad.ref_alignment].shape == (2, 5, 7) and not fd[wad.ref_alignment].any()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert not wad.feed_dict(ds, train=False)[wad.ref_alignment].any()     # no warning outside training


# ---- the binding table ------------------------------------------------------------------------------------------------------
def align_header_symbols():
    text = open(os.path.join(ROOT, "include", "nmhip_align.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nm_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


def test_align_header_matches_its_binding_table(lib):
    from neuralmonkey_amd import _lib
    from .test_abi import header_symbols
    mine = align_header_symbols()
    assert mine == set(_lib.ALIGN_SIGNATURES) == {"nm_align_xent", "nm_align_softmax"}
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("SIGNATURES") and n != "ALIGN_SIGNATURES"]
    assert len(others) >= 12 and all(not mine & set(table) for table in others)
    assert not mine & header_symbols()
    for name, (res, args) in _lib.ALIGN_SIGNATURES.items():
        fn = getattr(lib, name)                                          # exported, and bound by load()
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_align_entry_points_refuse_before_any_launch(lib):
    """Host buffers and a null stream: a call that got as far as a launch would fault or fail differently."""
    buf, tgt, pad = (ctypes.c_float * 4096)(), (ctypes.c_float * 4096)(), (ctypes.c_float * 64)()
    loss, dw = (ctypes.c_float * 64)(), (ctypes.c_float * 4096)()

    def xent(w=buf, t=3, b=2, s=5, target=tgt, sb=40, st=8, pad_=pad, loss_=loss, dw_=dw, acc=0):
        return lib.nm_align_xent(None, w, t, b, s, target, sb, st, pad_, None, loss_, dw_, acc)
    for kwargs, text in ((dict(w=None), b"nm_align_xent: null pointer"), (dict(target=None), b"nm_align_xent: null pointer"),
                         (dict(pad_=None), b"nm_align_xent: null pointer"), (dict(loss_=None), b"nm_align_xent: null pointer"),
                         (dict(t=-1), b"nm_align_xent: bad sizes T -1, B 2, S 5"), (dict(b=-2), b"nm_align_xent: bad sizes"),
                         (dict(s=-1), b"nm_align_xent: bad sizes"),
                         (dict(s=0), b"nm_align_xent: S = 0 source positions with 6 rows"),
                         (dict(st=4), b"nm_align_xent: tgt_stride_t 4 below S 5"),
                         (dict(sb=23), b"nm_align_xent: tgt_stride_b 23 below T * tgt_stride_t = 3 x 8"),
                         (dict(t=1 << 20, b=1 << 11, sb=1 << 40), b"nm_align_xent: T*B = 1048576 x 2048 rows beyond 2^31 - 1"),
                         (dict(t=1 << 40, b=1 << 40), b"rows beyond 2^31 - 1"),
                         (dict(dw_=buf), b"nm_align_xent: dw aliasing w")):
        assert xent(**kwargs) < 0 and text in lib.nm_last_error(), (kwargs, lib.nm_last_error())
    # T*B == 0 is a no-op, whatever else is passed
    assert xent(t=0, w=None, target=None, pad_=None, loss_=None, dw_=None) == 0
    assert xent(b=0, s=0, w=None, target=None, pad_=None, loss_=None) == 0

    def soft(w=buf, t=3, b=2, s=5, out=dw):
        return lib.nm_align_softmax(None, w, t, b, s, out)
    for kwargs, text in ((dict(w=None), b"nm_align_softmax: null pointer"), (dict(out=None), b"nm_align_softmax: null pointer"),
                         (dict(t=-1), b"nm_align_softmax: bad sizes"), (dict(s=0), b"nm_align_softmax: S = 0 source positions"),
                         (dict(t=1 << 31, b=1), b"nm_align_softmax: T*B = 2147483648 x 1 rows beyond 2^31 - 1"),
                         (dict(out=buf), b"nm_align_softmax: out aliasing w")):
        assert soft(**kwargs) < 0 and text in lib.nm_last_error(), (kwargs, lib.nm_last_error())
    assert soft(t=0, w=None, out=None) == 0 and soft(b=0, s=0) == 0


def test_kernels_of_the_align_file_do_not_spill(lib):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_resources
    finally:
        sys.path.pop(0)
    mine = {k: v for k, v in kernel_resources().items() if "align_xent_kernel" in k or "align_softmax_kernel" in k}
    assert len(mine) == 2, sorted(mine)
    assert all(v["scratch"] == 0 and v["lds"] == 0 and v["max_threads"] == 256 for v in mine.values())
