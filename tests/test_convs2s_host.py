"""The convolutional sequence-to-sequence encoder without a GPU: the reference's tests/bpe.ini built from the committed
archives, the archive's bytes, constructor parameters and refusals, the declared variables against the names and shapes
the reference created, the fixtures of tests/golden/convs2s, and the fifth binding table (include/nmhip_convs2s.h) with
its refusals."""
import ctypes
import glob
import json
import os
import re
import tarfile

import numpy as np
import pytest

from . import convs2s_models as M

from .test_reference_inis import REF        # noqa: E402  (the reference tree, where there is one)

ROOT = M.ROOT
MEMBERS = {"tests/bpe.ini", "tests/data/merges_100.bpe", "tests/data/bpe_vocab.tsv"}


# ---- through the config loader ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bpe_root(tmp_path_factory):
    """tests/bpe.ini and the two word lists it names, plus the corpora of the first archive."""
    root = tmp_path_factory.mktemp("reference_tests_convs2s")
    for bundle in (os.path.join(M.GOLDEN, "reference_tests.tar.gz"), M.BUNDLE):
        with tarfile.open(bundle) as tar:
            tar.extractall(root)
    return str(root)


def test_bpe_ini_builds_unmodified(bpe_root):
    """Fails on a tree without the feature with SymbolNotShipped."""
    from .test_reference_inis import load_verbatim
    model = load_verbatim(bpe_root, "bpe", initialize=False, device="cpu")
    from neuralmonkey_amd.attention import Attention
    from neuralmonkey_amd.decoders import Decoder
    from neuralmonkey_amd.encoders import SentenceEncoder as RecurrentSentenceEncoder
    from neuralmonkey_amd.encoders.facebook_conv import SentenceEncoder
    from neuralmonkey_amd.model.sequence import EmbeddedSequence
    from neuralmonkey_amd.runners import GreedyRunner
    runner, = model.runners
    dec = runner.decoder
    assert isinstance(runner, GreedyRunner) and isinstance(dec, Decoder) and runner.output_series == "target_greedy"
    enc, = dec.encoders
    assert type(enc) is SentenceEncoder and SentenceEncoder is not RecurrentSentenceEncoder    # the bare name stays
    assert enc.name == "sentence_encoder" and isinstance(enc.input_sequence, EmbeddedSequence)
    assert (enc.conv_features, enc.encoder_layers, enc.kernel_width, enc.dropout_keep_prob) == (10, 2, 5, 0.5)
    assert (enc.dimension, enc.output_size, enc.max_input_length) == (10, 10, 10)
    assert enc.input_sequence.embedding_sizes == [11] and enc.input_sequence.data_id == "source_bpe"
    att, = dec.attentions
    assert isinstance(att, Attention) and att.encoder is enc
    assert enc.has_time_loop is False and enc.graph_safe_training(True) is True
    assert enc.temporal_mask.key != enc.input_sequence.temporal_mask.key       # its own tensor, the sequence's values
    assert model.trainers[0].objectives[0].decoder is dec
    batch = next(iter(model.train_dataset.batches()))
    fd = enc.input_sequence.feed_dict(batch, train=True)
    ids, = [v for v in fd.values() if isinstance(v, np.ndarray) and v.ndim == 2]
    assert ids.shape[1] <= 10                                                   # max_length cuts the BPE sentences


def test_archive_members_are_the_references_bytes(bpe_root):
    with tarfile.open(M.BUNDLE) as tar:
        names = [m.name for m in tar.getmembers()]
    assert set(names) == MEMBERS and len(names) == 3
    assert os.path.getsize(M.BUNDLE) < 8 * 1024
    if os.path.isdir(REF):
        for rel in names:
            with open(os.path.join(REF, rel), "rb") as a, open(os.path.join(bpe_root, rel), "rb") as b:
                assert a.read() == b.read(), rel


# ---- signatures and argument checks --------------------------------------------------------------------------------------
def test_constructor_parameters_are_the_references():
    from .test_reference_signatures import product_parameters, read_reference_parameters
    path, name = "encoders/facebook_conv.py", "SentenceEncoder"
    with open(M.LISTS, encoding="utf-8") as handle:
        lists = json.load(handle)
    assert list(lists) == [path] and list(lists[path]) == [name]
    want = [tuple(p) for p in lists[path][name]]
    assert [p[0] for p in want] == ["name", "input_sequence", "conv_features", "encoder_layers", "kernel_width",
                                    "dropout_keep_prob", "reuse", "save_checkpoint", "load_checkpoint", "initializers"]
    if os.path.isdir(REF):
        assert read_reference_parameters(path, name) == want
    assert product_parameters(path, name) == want


def test_constructor_defaults_and_refusals_use_the_references_words():
    import inspect
    from neuralmonkey_amd.encoders.facebook_conv import SentenceEncoder
    from neuralmonkey_amd.model.sequence import EmbeddedSequence
    from neuralmonkey_amd.model.stateful import TemporalStatefulWithOutput
    from neuralmonkey_amd.runtime import reset_registry
    defaults = {k: p.default for k, p in inspect.signature(SentenceEncoder.__init__).parameters.items()}
    assert (defaults["kernel_width"], defaults["dropout_keep_prob"]) == (5, 1.0)
    assert "never applied" in SentenceEncoder.__init__.__doc__
    reset_registry()
    seq = EmbeddedSequence("seq", M.words(3), "source", 4, max_length=6)
    enc = SentenceEncoder("enc", seq, 8, 2)
    assert isinstance(enc, TemporalStatefulWithOutput) and (enc.dimension, enc.output_size) == (8, 8)
    assert enc.max_input_length == 6 and enc.kernel_width == 5
    for features in (0, -3):
        with pytest.raises(ValueError, match=r"^Number of features must be a positive integer\.$"):
            SentenceEncoder("enc2", seq, features, 2)
    for layers in (0, -1):
        with pytest.raises(ValueError, match=r"^Number of encoder layers must be a positive integer\.$"):
            SentenceEncoder("enc3", seq, 8, layers)
    unbounded = EmbeddedSequence("seq2", M.words(3), "source", 4)
    with pytest.raises(ValueError, match=r"^Input sequence must have a maximum length for positional embeddings with "
                                         r"this encoder$"):
        SentenceEncoder("enc4", unbounded, 8, 2)
    with pytest.raises(TypeError):
        SentenceEncoder("enc5", seq, "8", 2)
    with pytest.raises(TypeError):
        SentenceEncoder("enc6", "seq", 8, 2)
    with pytest.raises(TypeError):
        SentenceEncoder("enc7", seq, 8, 2, kernel_width=2.5)
    if os.path.isdir(REF):                                      # the three messages are the reference's own text
        text = re.sub(r'"\s*\n\s*"', "", open(os.path.join(REF, "neuralmonkey/encoders/facebook_conv.py")).read())
        for message in ("Number of features must be a positive integer.",
                        "Number of encoder layers must be a positive integer.",
                        "Input sequence must have a maximum length for positional embeddings with this encoder"):
            assert message in text, message


# ---- variables -------------------------------------------------------------------------------------------------------------
def declared(enc, seq):
    from neuralmonkey_amd.variables import VariableStore
    store = VariableStore("cpu", seed=3)
    seq.declare_variables(store)
    enc.declare_variables(store)
    return store


def recorded_variables(z):
    return {str(n): tuple(json.loads(str(s))) for n, s in zip(z["out/variable_names"], z["out/variable_shapes"])}


@pytest.mark.parametrize("case", M.FORWARD_CASES)
def test_declared_variables_are_the_ones_the_reference_created(case):
    z, cfg, params = M.load_fixture(case)
    want = recorded_variables(z)
    assert want == {n: tuple(v.shape) for n, v in params.items()}
    seq, enc, avg, dec = M.build_parts(cfg)
    store = declared(enc, seq)
    mine = {n: s.shape for n, s in store.specs.items()}
    assert mine == {n: s for n, s in want.items() if n.split("/")[0] in ("encoder", "encoder_input")}
    assert len([n for n in mine if n.startswith("encoder/")]) == 5 + 2 * cfg["encoder_layers"]


def test_declared_variables_of_bpe_ini_follow_the_recorded_pattern(bpe_root):
    """E = 11, C = 10, L = 2, max_length = 10: the fixtures' names with this configuration's sizes."""
    from .test_reference_inis import load_verbatim
    model = load_verbatim(bpe_root, "bpe", initialize=False, device="cpu")
    enc = model.runners[0].decoder.encoders[0]
    store = declared(enc, enc.input_sequence)
    mine = {n: s.shape for n, s in store.specs.items() if n.startswith("sentence_encoder/")}
    z, cfg, _ = M.load_fixture("convs2s_k5")
    assert (cfg["emb"], cfg["conv_features"], cfg["encoder_layers"], cfg["kernel_width"], cfg["max_length"]) == (
        6, 10, 2, 5, 9)
    resize = {6: 11, 9: 10}                                                    # E and max_length; C, L and w agree
    want = {"sentence_encoder/" + n[len("encoder/"):]: tuple(resize.get(d, d) for d in s)
            for n, s in recorded_variables(z).items() if n.startswith("encoder/")}
    assert mine == want
    assert mine["sentence_encoder/input_projection/order_embeddings"] == (10, 11)
    assert mine["sentence_encoder/encoder_conv_1/convolution_filters"] == (5, 10, 20)


def test_initializers_are_the_references():
    """Order embeddings and dense kernels: glorot uniform; filters: normal with stddev sqrt(4 / C); biases: zeros."""
    from neuralmonkey_amd.encoders.facebook_conv import SentenceEncoder
    from neuralmonkey_amd.model.sequence import EmbeddedSequence
    from neuralmonkey_amd.runtime import reset_registry
    reset_registry()
    seq = EmbeddedSequence("seq", M.words(3), "source", 40, max_length=50)
    enc = SentenceEncoder("enc", seq, 64, 1, kernel_width=3)
    store = declared(enc, seq)
    store.finalize()
    v = {n: store[n].numpy() for n in store.names()}
    for name, (fan_in, fan_out) in (("enc/input_projection/order_embeddings", (50, 40)),
                                    ("enc/order_and_embed/kernel", (40, 64)),
                                    ("enc/input_to_final_state/kernel", (40, 64))):
        lim = np.sqrt(6.0 / (fan_in + fan_out))
        assert np.abs(v[name]).max() <= lim and np.abs(v[name]).max() > 0.9 * lim, name
        assert abs(v[name].std() - lim / np.sqrt(3.0)) < 0.1 * lim, name
    filt = v["enc/encoder_conv_0/convolution_filters"]
    assert filt.shape == (3, 64, 128) and abs(filt.std() - np.sqrt(4 / 64)) < 0.02 * np.sqrt(4 / 64)
    assert abs(filt.mean()) < 0.01 and np.abs(filt).max() > 3 * np.sqrt(4 / 64)            # normal, not uniform
    for name in ("enc/order_and_embed/bias", "enc/input_to_final_state/bias", "enc/encoder_conv_0/conv_bias"):
        assert not v[name].any(), name


# ---- the fixtures ----------------------------------------------------------------------------------------------------------
def ref_conv1d(x, w):
    width, steps = w.shape[0], x.shape[1]
    before = (width - 1) // 2
    padded = np.pad(x, ((0, 0), (before, width - 1 - before), (0, 0)))
    return sum(padded[:, k:k + steps] @ w[k] for k in range(width))


def test_fixture_directory_holds_the_issues_cases():
    have = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(M.FIX, "*.npz")))
    assert have == sorted(M.FORWARD_CASES)
    want = {"convs2s_k5": (5, 2, 10, 9, 7), "convs2s_k4_one_layer": (4, 1, 7, 9, 7),
            "convs2s_k3_truncated": (3, 3, 10, 5, 5), "convs2s_classifier": (5, 2, 10, 9, 7),
            "fd_gradients_convs2s": (5, 2, 10, 9, 7)}
    for case in M.FORWARD_CASES:
        z, cfg, params = M.load_fixture(case)
        steps = z["out/temporal_states"].shape[1]
        assert (cfg["kernel_width"], cfg["encoder_layers"], cfg["conv_features"], cfg["max_length"], steps) == want[case]
        assert cfg["emb"] == 6 and cfg["src_vocab"] == 17
        sentences = [str(s).split(" ") for s in z["in/src_sentences"]]
        assert [len(s) for s in sentences] == M.LENGTHS and any("never-seen" in s for s in sentences)
        assert z["out/temporal_mask"].sum(axis=1).astype(int).tolist() == [min(n, steps) for n in M.LENGTHS]
        assert z["out/ordered_embedded_inputs"].shape == (5, steps, 6) and z["out/output"].shape == (
            5, cfg["conv_features"])
        assert os.path.getsize(os.path.join(M.FIX, case + ".npz")) < 64 * 1024
        # padded positions carry the bare order embedding, and the maximum runs over them too
        table = params["encoder/input_projection/order_embeddings"]
        pad = z["out/temporal_mask"] == 0
        assert np.array_equal(z["out/ordered_embedded_inputs"][pad], np.broadcast_to(table[:steps], (5, steps, 6))[pad])
        assert np.array_equal(z["out/output"], z["out/temporal_states"].max(axis=1))
    assert sum(n > 5 for n in M.LENGTHS) == 2                                   # two sentences cut by max_length = 5
    for case in M.FD_CASES:
        z, cfg, params = M.load_fixture(case)
        names = [str(n) for n in z["fd/names"]]
        assert set(names) == set(params) and float(z["fd/h"]) == 5e-3
        assert all(names.count(n) == min(4, params[n].size) for n in params)


@pytest.mark.parametrize("case", M.FORWARD_CASES)
def test_numpy_restatement_reproduces_the_reference(case):
    """The formulas the kernels implement, in float64 NumPy, from the fixture's variables."""
    z, cfg, params = M.load_fixture(case)
    p = {n: v.astype(np.float64) for n, v in params.items()}
    inp = z["out/ordered_embedded_inputs"].astype(np.float64)
    x = inp @ p["encoder/order_and_embed/kernel"] + p["encoder/order_and_embed/bias"]
    c = cfg["conv_features"]
    for i in range(cfg["encoder_layers"]):
        pre = "encoder/encoder_conv_{}/".format(i)
        zz = ref_conv1d(x, p[pre + "convolution_filters"]) + p[pre + "conv_bias"]
        x = zz[..., :c] / (1.0 + np.exp(-zz[..., c:])) + x
    states = x + inp @ p["encoder/input_to_final_state/kernel"] + p["encoder/input_to_final_state/bias"]
    scale = float(np.abs(z["out/temporal_states"]).max())
    assert np.abs(states - z["out/temporal_states"]).max() <= 1e-5 * scale


# ---- the fifth binding table ----------------------------------------------------------------------------------------------
def convs2s_header_symbols():
    text = open(os.path.join(ROOT, "include", "nmhip_convs2s.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nm_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


def test_convs2s_header_matches_its_binding_table(lib):
    from neuralmonkey_amd import _lib
    from .test_abi import header_symbols
    from .test_ctc_host import ctc_header_symbols
    from .test_labeler_host import label_header_symbols
    from .test_pool_host import pool_header_symbols
    mine = convs2s_header_symbols()
    assert mine == set(_lib.CONVS2S_SIGNATURES) and len(mine) == 3
    for other in (_lib.SIGNATURES, _lib.CTC_SIGNATURES, _lib.LABEL_SIGNATURES, _lib.POOL_SIGNATURES):
        assert not mine & set(other)
    assert not mine & header_symbols() and not mine & ctc_header_symbols() and not mine & label_header_symbols()
    assert not mine & pool_header_symbols()
    for name, (res, args) in _lib.CONVS2S_SIGNATURES.items():
        fn = getattr(lib, name)                                          # exported, and bound by load()
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    header = open(os.path.join(ROOT, "include", "nmhip_convs2s.h")).read()
    assert "facebook_conv.py:102-121" in header and "nn/projection.py:60-75" in header      # the lines it replaces


def test_convs2s_entry_points_refuse_before_any_launch(lib):
    """Host buffers and a null stream: a call that got as far as a launch would fault or fail differently."""
    buf = (ctypes.c_float * 8192)()
    other = (ctypes.c_float * 8192)()
    third = (ctypes.c_float * 8192)()
    save = (ctypes.c_float * 8192)()

    def fwd(x=buf, ldx=8, b=2, t=3, c=8, w=5, filt=third, bias=third, y=other, ldy=8, lin=None, sig=None, algo=0):
        return lib.nm_conv1d_glu_fwd(None, x, ldx, b, t, c, w, filt, bias, y, ldy, lin, sig, algo)
    for kwargs, text in ((dict(b=0), b"nm_conv1d_glu_fwd: bad sizes B 0, T 3, C 8, w 5"),
                         (dict(t=0), b"nm_conv1d_glu_fwd: bad sizes B 2, T 0, C 8, w 5"),
                         (dict(c=0), b"nm_conv1d_glu_fwd: bad sizes B 2, T 3, C 0, w 5"),
                         (dict(w=0), b"nm_conv1d_glu_fwd: bad sizes B 2, T 3, C 8, w 0"),
                         (dict(b=1 << 20, t=1 << 12), b"nm_conv1d_glu_fwd: B*T = 4294967296 rows beyond 2^31"),
                         (dict(b=(1 << 31) - 1, t=1, c=1 << 22),
                          b"nm_conv1d_glu_fwd: grid of 2147483647 x 131072 workgroups beyond the launch limits"),
                         (dict(ldx=7), b"nm_conv1d_glu_fwd: ldx 7 below C 8"),
                         (dict(ldy=7), b"nm_conv1d_glu_fwd: ldy 7 below C 8"),
                         (dict(x=None), b"nm_conv1d_glu_fwd: null pointer"),
                         (dict(filt=None), b"nm_conv1d_glu_fwd: null pointer"),
                         (dict(bias=None), b"nm_conv1d_glu_fwd: null pointer"),
                         (dict(y=None), b"nm_conv1d_glu_fwd: null pointer"),
                         (dict(y=buf), b"nm_conv1d_glu_fwd: y aliasing x (a tile reads its neighbours' rows of x as halo)"),
                         (dict(y=ctypes.byref(buf, 4 * 40)),
                          b"nm_conv1d_glu_fwd: y aliasing x (a tile reads its neighbours' rows of x as halo)"),
                         (dict(lin=save), b"nm_conv1d_glu_fwd: lin_save and sig_save come together or not at all"),
                         (dict(sig=save), b"nm_conv1d_glu_fwd: lin_save and sig_save come together or not at all"),
                         (dict(algo=3), b"nm_conv1d_glu_fwd: algo 3 (0 auto, 1 mfma, 2 scalar)"),
                         (dict(algo=-1), b"nm_conv1d_glu_fwd: algo -1 (0 auto, 1 mfma, 2 scalar)"),
                         (dict(algo=1, w=9), b"nm_conv1d_glu_fwd: the MFMA kernel takes widths <= 8, not 9")):
        assert fwd(**kwargs) < 0 and lib.nm_last_error() == text, (kwargs, lib.nm_last_error())

    assert lib.nm_conv1d_glu_workspace_bytes(2, 3, 8, 5) == 5 * 8 * 16 * 4            # one slab of [w, C, 2C]
    assert lib.nm_conv1d_glu_workspace_bytes(16, 256, 512, 5) > 5 * 512 * 1024 * 4    # several position slices
    for bad in ((0, 3, 8, 5), (2, 0, 8, 5), (2, 3, 0, 5), (2, 3, 8, 0), (1 << 31, 3, 8, 5)):
        assert lib.nm_conv1d_glu_workspace_bytes(*bad) == 0
    # the slab plan of the shared weight gradient (tests/conv1d_ref.py): the GPU cases G1-G3 take two to four slabs, the
    # largest of the older cases (2 x 131, C 200, w 5) one
    from .conv1d_ref import GLU_SLAB_CASES, glu_filters, slab_plan
    for name, ((bsz, steps, c, width), tiles, slices, per, last) in GLU_SLAB_CASES.items():
        plan = slab_plan(bsz, steps, c, glu_filters(c, width))
        assert (plan["tiles"], plan["slices"], plan["per"], plan["last"]) == (tiles, slices, per, last), (name, plan)
        assert lib.nm_conv1d_glu_workspace_bytes(bsz, steps, c, width) == slices * width * c * 2 * c * 4, name
    assert all(GLU_SLAB_CASES[name][3] == GLU_SLAB_CASES[name][0][1] for name in ("G2", "G3"))    # seams on sentence seams
    assert slab_plan(2, 131, 200, glu_filters(200, 5))["slices"] == 1
    assert lib.nm_conv1d_glu_workspace_bytes(2, 131, 200, 5) == 5 * 200 * 400 * 4

    def bwd(x=buf, ldx=8, b=2, t=3, c=8, w=5, filt=third, lin=save, sig=save, dy=other, lddy=8, dz=third, dx=None,
            lddx=8, acc=0, dw=None, db=None, accp=0, ws=None, ws_bytes=0, algo=0):
        dx = ctypes.byref(other, 4 * 1024) if dx is None else dx
        return lib.nm_conv1d_glu_bwd(None, x, ldx, b, t, c, w, filt, lin, sig, dy, lddy, dz, dx, lddx, acc, dw, db, accp,
                                     ws, ws_bytes, algo)
    for kwargs, text in ((dict(c=0), b"nm_conv1d_glu_bwd: bad sizes B 2, T 3, C 0, w 5"),
                         (dict(b=1 << 20, t=1 << 12), b"nm_conv1d_glu_bwd: B*T = 4294967296 rows beyond 2^31"),
                         (dict(ldx=7), b"nm_conv1d_glu_bwd: ldx 7 below C 8"),
                         (dict(lddy=7), b"nm_conv1d_glu_bwd: lddy 7 below C 8"),
                         (dict(lddx=7), b"nm_conv1d_glu_bwd: lddx 7 below C 8"),
                         (dict(x=None), b"nm_conv1d_glu_bwd: null pointer"),
                         (dict(filt=None), b"nm_conv1d_glu_bwd: null pointer"),
                         (dict(lin=None), b"nm_conv1d_glu_bwd: null pointer"),
                         (dict(sig=None), b"nm_conv1d_glu_bwd: null pointer"),
                         (dict(dy=None), b"nm_conv1d_glu_bwd: null pointer"),
                         (dict(dz=None), b"nm_conv1d_glu_bwd: null pointer"),
                         (dict(dx=other), b"nm_conv1d_glu_bwd: dx aliasing dy"),
                         (dict(dx=ctypes.byref(other, 4 * 40)), b"nm_conv1d_glu_bwd: dx aliasing dy"),
                         (dict(algo=4), b"nm_conv1d_glu_bwd: algo 4 (0 auto, 1 mfma, 2 scalar)"),
                         (dict(algo=1, w=9), b"nm_conv1d_glu_bwd: the MFMA kernels take widths <= 8, not 9"),
                         (dict(dw=save), b"nm_conv1d_glu_bwd: the weight gradient needs a workspace"),
                         (dict(dw=save, ws=third, ws_bytes=2559),
                          b"nm_conv1d_glu_bwd: workspace too small (2559 < 2560 bytes)")):
        assert bwd(**kwargs) < 0 and lib.nm_last_error() == text, (kwargs, lib.nm_last_error())


def test_kernels_of_the_convs2s_layer_do_not_spill(lib):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_resources
    finally:
        sys.path.pop(0)
    mine = {k: v for k, v in kernel_resources().items() if "convs2s_" in k}
    assert len(mine) == 4, sorted(mine)
    assert all(v["scratch"] == 0 for v in mine.values())
    mfma, = [v for k, v in mine.items() if "convs2s_glu_mfma" in k]
    assert mfma["lds"] == 41472
