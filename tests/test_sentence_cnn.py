"""SentenceCNNEncoder without a GPU: the reference's own constructor test runs against the product, the constructor
has the reference's parameters, tests/small_sent_cnn.ini loads byte for byte from its bundle and declares the
variables the reference's graph holds, the new C entry points refuse bad arguments before any launch, and the weight
gradient's slab plan is the one the GPU cases of tests/conv1d_ref.py name."""
import ctypes
import os
import tarfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BUNDLE_CNN = os.path.join(HERE, "golden", "reference_tests_cnn.tar.gz")     # tests/small_sent_cnn.ini + its vocabulary
BUNDLE = os.path.join(HERE, "golden", "reference_tests.tar.gz")             # the corpora it names
REF = "/root/reference"


@pytest.fixture(scope="module")
def cnn_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("reference_tests_cnn")
    for bundle in (BUNDLE, BUNDLE_CNN):
        with tarfile.open(bundle) as tar:
            tar.extractall(root)
    return str(root)


def test_both_import_paths_resolve():
    import importlib
    from neuralmonkey_amd import encoders
    # (by module name: a placeholder of the reference-unittest alias may have shadowed the package attribute)
    module = importlib.import_module("neuralmonkey_amd.encoders.sentence_cnn_encoder")
    assert encoders.SentenceCNNEncoder is module.SentenceCNNEncoder


def test_the_references_constructor_test_passes_on_the_product(monkeypatch):
    from . import test_reference_unittests as T
    if not os.path.isdir(T.TESTS):
        pytest.skip("no reference tree on this machine")
    from neuralmonkey_amd.runtime import reset_registry
    monkeypatch.setattr(T, "PLACEHOLDERS", {})
    reset_registry()
    result, log = T.run_reference_tests("test_encoders_init", only=("test_sentence_cnn_encoder",))
    assert result.testsRun == 1, log
    assert not result.failures and not result.errors, log


def test_constructor_parameters_are_the_references():
    from .test_reference_signatures import product_parameters, read_reference_parameters
    path = "encoders/sentence_cnn_encoder.py"
    if not os.path.isdir(REF):
        pytest.skip("no reference tree on this machine")
    want = read_reference_parameters(path, "SentenceCNNEncoder")
    assert product_parameters(path, "SentenceCNNEncoder") == want


def _sequence():
    from neuralmonkey_amd.model.sequence import EmbeddedSequence
    from neuralmonkey_amd.vocabulary import Vocabulary
    return EmbeddedSequence("seq", Vocabulary(["a", "b", "c"]), "chars", 11)


@pytest.mark.parametrize("kw,error", [
    ({"dropout_keep_prob": 0.0}, ValueError), ({"dropout_keep_prob": 1.5}, ValueError),
    ({"rnn_size": 0}, ValueError), ({"highway_depth": 0}, ValueError), ({"segment_size": 0}, ValueError),
    ({"filters": []}, ValueError), ({"filters": [(0, 3)]}, ValueError), ({"filters": [(2, 0)]}, ValueError),
    ({"filters": [(2, 3, 4)]}, TypeError), ({"segment_size": 2.5}, TypeError), ({"rnn_size": "7"}, TypeError),
])
def test_constructor_refuses_what_the_reference_refuses(kw, error):
    from neuralmonkey_amd.encoders import SentenceCNNEncoder
    from neuralmonkey_amd.runtime import reset_registry
    reset_registry()
    args = dict(name="cnn", input_sequence=_sequence(), segment_size=5, highway_depth=2, rnn_size=7,
                filters=[(1, 4), (2, 4)])
    args.update(kw)
    with pytest.raises(error):
        SentenceCNNEncoder(**args)


def test_noisy_activations_construct_and_refuse_when_run():
    from neuralmonkey_amd.encoders import SentenceCNNEncoder
    from neuralmonkey_amd.runtime import reset_registry
    reset_registry()
    enc = SentenceCNNEncoder("cnn_noisy", _sequence(), 5, 2, 7, [(1, 4)], use_noisy_activations=True)
    with pytest.raises(NotImplementedError, match="NoisyGRUCell"):
        enc._activations.fn(enc, None)               # what every output of the encoder is computed from


# the variables tf.get_variable creates for tests/small_sent_cnn.ini's [encoder] (sentence_cnn_encoder.py:118-124,
# nn/highway.py:37-44, tf.nn.bidirectional_dynamic_rnn's scopes around OrthoGRUCell): E = 11, filters 3 x 13,
# highway depth 3, GRU 7
SMALL_SENT_CNN_VARIABLES = dict(
    [("conv-maxpool-{}/conv_W".format(w), (w, 11, 13)) for w in (1, 2, 3)]
    + [("conv-maxpool-{}/conv_bias".format(w), (13,)) for w in (1, 2, 3)]
    + [("highway_layer_{}/{}".format(i, n), (39, 39) if n.startswith("weight") else (39,))
       for i in range(3) for n in ("weight_H", "bias_H", "weight_T", "bias_T")]
    + [("bidirectional_rnn/{}/OrthoGRUCell/{}".format(d, n), s) for d in ("fw", "bw")
       for n, s in (("gates/kernel", (46, 14)), ("gates/bias", (14,)), ("candidate/kernel", (46, 7)),
                    ("candidate/bias", (7,)))])


def test_small_sent_cnn_ini_loads_verbatim_with_the_references_variables(cnn_root):
    from .test_reference_inis import load_verbatim
    from neuralmonkey_amd.encoders import SentenceCNNEncoder
    model = load_verbatim(cnn_root, "small_sent_cnn", device="cpu")
    enc = model.runners[0].decoder.encoders[0]
    assert isinstance(enc, SentenceCNNEncoder)
    assert (enc.segment_size, enc.highway_depth, enc.rnn_size, enc.filters) == (5, 3, 7, [(1, 13), (2, 13), (3, 13)])
    store = model.tf_manager.sessions[0].store
    mine = {n.split("/", 1)[1]: tuple(store[n].shape) for n in store.names() if n.startswith("sentence_encoder/")}
    assert mine == SMALL_SENT_CNN_VARIABLES
    for w in (1, 2, 3):                          # variance_scaling(fan_avg, uniform) with TF's rank-3 fans
        lim = (3.0 / ((w * 11 + w * 13) / 2.0)) ** 0.5
        vals = store["sentence_encoder/conv-maxpool-{}/conv_W".format(w)]
        assert float(vals.abs().max()) <= lim and float(vals.abs().max()) > 0.5 * lim
    for i in range(3):
        assert float(store["sentence_encoder/highway_layer_{}/bias_T".format(i)].max()) == -1.0
    if os.path.isdir(REF):
        with open(os.path.join(REF, "tests", "small_sent_cnn.ini"), "rb") as a, \
                open(os.path.join(cnn_root, "tests", "small_sent_cnn.ini"), "rb") as b:
            assert a.read() == b.read()


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


def test_conv_entry_points_validate_before_any_launch(lib):
    buf = (ctypes.c_float * 64)()
    ibuf = (ctypes.c_int * 64)()
    widths, counts = (ctypes.c_int * 2)(1, 2), (ctypes.c_int * 2)(3, 4)
    ptrs = (ctypes.c_void_p * 2)(ctypes.addressof(buf), ctypes.addressof(buf))
    rc = lib.nm_conv1d_pool_fwd(None, buf, 4, 2, 6, 4, 0, 2, widths, counts, ptrs, ptrs, buf, ibuf, 7, None, None, None,
                                None, 0)
    assert rc < 0 and b"bad sizes" in lib.nm_last_error()
    rc = lib.nm_conv1d_pool_fwd(None, buf, 4, 2, 6, 4, 5, 2, widths, counts, ptrs, ptrs, buf, ibuf, 8, None, None, None,
                                None, 0)
    assert rc < 0 and b"sum of filter counts" in lib.nm_last_error()
    rc = lib.nm_conv1d_pool_fwd(None, None, 4, 2, 6, 4, 5, 2, widths, counts, ptrs, ptrs, buf, ibuf, 7, None, None,
                                None, None, 0)
    assert rc < 0 and b"null operand" in lib.nm_last_error()
    bad = (ctypes.c_int * 2)(1, 0)
    rc = lib.nm_conv1d_pool_fwd(None, buf, 4, 2, 6, 4, 5, 2, widths, bad, ptrs, ptrs, buf, ibuf, 1, None, None, None,
                                None, 0)
    assert rc < 0 and b"count 0" in lib.nm_last_error()
    wide = (ctypes.c_int * 2)(1, 9)
    rc = lib.nm_conv1d_pool_fwd(None, buf, 4, 2, 6, 4, 5, 2, wide, counts, ptrs, ptrs, buf, ibuf, 7, None, None, None,
                                None, 1)
    assert rc < 0 and b"MFMA kernel takes" in lib.nm_last_error()
    # the weight-gradient workspace: fixed-order slabs of whole filter banks
    slab = 1 * 4 * 3 + 2 * 4 * 4
    nbytes = lib.nm_conv1d_wgrad_workspace_bytes(2, 6, 4, 2, widths, counts)
    assert nbytes > 0 and nbytes % (4 * slab) == 0
    assert lib.nm_conv1d_wgrad_workspace_bytes(0, 6, 4, 2, widths, counts) == 0
    rc = lib.nm_conv1d_pool_bwd(None, buf, 4, 2, 6, 4, 5, 2, widths, counts, ptrs, buf, ibuf, buf, 7, buf, buf, 0, ptrs,
                                ptrs, 1, buf, 4, 0)
    assert rc < 0 and b"workspace too small" in lib.nm_last_error()
    rc = lib.nm_conv1d_pool_bwd(None, buf, 4, 2, 6, 4, 5, 2, widths, counts, ptrs, buf, ibuf, None, 7, buf, buf, 0, None,
                                None, 1, None, 0, 0)
    assert rc < 0 and b"null operand" in lib.nm_last_error()
    rc = lib.nm_highway_fwd(None, buf, buf, 4, buf, 4, buf, buf, buf, buf, buf, 2, 4)
    assert rc < 0 and b"may not overwrite" in lib.nm_last_error()
    rc = lib.nm_highway_fwd(None, buf, buf, 2, buf, 4, buf, buf, None, buf, buf, 2, 4)
    assert rc < 0 and b"nm_highway_fwd" in lib.nm_last_error()
    rc = lib.nm_highway_bwd(None, buf, buf, 4, buf, buf, buf, buf, 2, buf, 2, 4, 0)
    assert rc < 0 and b"bad shape" in lib.nm_last_error()


def _tables(filters):
    n = len(filters)
    return (ctypes.c_int * n)(*[w for w, _ in filters]), (ctypes.c_int * n)(*[c for _, c in filters])


# the largest shape of tests/test_sentence_cnn_gpu.py's first table: one slab, like every shape of that table
LARGEST_ONE_SLAB_CASE = (2, 250, 128, [(2, 13), (7, 300)])


def test_the_slab_plan_of_the_weight_gradient_is_the_one_the_gpu_cases_claim(lib):
    """nm_conv1d_wgrad_workspace_bytes == slices * slab * 4 with the slab counts tests/conv1d_ref.py's table names: the
    GPU cases P1-P6 cross the thresholds they say they cross, and the older cases never did."""
    from .conv1d_ref import POOL_SLAB_CASES, slab_plan
    for name, ((bsz, slen, e, filters), tiles, slices, per, last) in POOL_SLAB_CASES.items():
        plan = slab_plan(bsz, slen, e, filters)
        assert (plan["tiles"], plan["slices"], plan["per"], plan["last"]) == (tiles, slices, per, last), (name, plan)
        widths, counts = _tables(filters)
        slab = sum(w * e * n for w, n in filters)
        assert lib.nm_conv1d_wgrad_workspace_bytes(bsz, slen, e, len(filters), widths, counts) == slices * slab * 4, name
    limits = {name: slab_plan(*case[0])["limit"] for name, case in POOL_SLAB_CASES.items()}
    assert limits == {"P1": "positions", "P2": "positions", "P3": "tiles", "P4": "cap", "P5": "positions",
                      "P6": "positions"}
    assert POOL_SLAB_CASES["P4"][4] % 32 != 0 and POOL_SLAB_CASES["P1"][3] % 32 != 0       # partial last LDS stages
    assert POOL_SLAB_CASES["P2"][3] % POOL_SLAB_CASES["P2"][0][1] != 0                     # a seam mid-sentence
    bsz, slen, e, filters = LARGEST_ONE_SLAB_CASE
    widths, counts = _tables(filters)
    assert slab_plan(bsz, slen, e, filters)["slices"] == 1
    assert lib.nm_conv1d_wgrad_workspace_bytes(bsz, slen, e, 2, widths, counts) == (2 * 13 + 7 * 300) * 128 * 4


def test_sixteen_filter_widths_are_accepted_and_seventeen_refused(lib):
    from .conv1d_ref import W16
    buf = (ctypes.c_float * 64)()
    ibuf = (ctypes.c_int * 64)()
    for nw in (16, 17):
        filters = (W16 + [(1, 13)])[:nw]
        widths, counts = _tables(filters)
        ptrs = (ctypes.c_void_p * nw)(*[ctypes.addressof(buf)] * nw)
        # a pooled width that is one short: the refusal that follows the width count's, so no launch either way
        rc = lib.nm_conv1d_pool_fwd(None, buf, 11, 2, 6, 11, 5, nw, widths, counts, ptrs, ptrs, buf, ibuf, 13 * nw - 1,
                                    None, None, None, None, 0)
        assert rc < 0
        nbytes = lib.nm_conv1d_wgrad_workspace_bytes(4, 2000, 11, nw, widths, counts)
        if nw == 16:
            assert b"sum of filter counts" in lib.nm_last_error()
            assert nbytes == 29 * 72 * 11 * 13 * 4
        else:
            assert b"17 filter widths (1..16)" in lib.nm_last_error()
            assert nbytes == 0
        rc = lib.nm_conv1d_pool_bwd(None, buf, 11, 2, 6, 11, 5, nw, widths, counts, ptrs, buf, ibuf, buf, 13 * nw - 1,
                                    buf, buf, 0, None, None, 1, None, 0, 0)
        assert rc < 0 and (b"sum of filter counts" if nw == 16 else b"17 filter widths (1..16)") in lib.nm_last_error()
