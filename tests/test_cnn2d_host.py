"""The image encoder without a GPU: the reference's tests/str.ini built from the committed archive with NumPy images in
place of its image reader, the archive's bytes, constructor parameters and refusals, the declared variables against the
names and shapes the reference created, the fixtures of tests/golden/cnn2d and their NumPy restatement, the checkpoint
round trip of the moving statistics, and the sixth binding table (include/nmhip_image.h) with its refusals."""
import ctypes
import glob
import json
import os
import re
import tarfile

import numpy as np
import pytest

from . import cnn2d_models as M

from .test_reference_inis import REF        # noqa: E402  (the reference tree, where there is one)

ROOT = M.ROOT
MEMBERS = {"tests/str.ini", "tests/data/str/vocab.tsv", "tests/data/str/train_files.txt",
           "tests/data/str/train_words.txt", "tests/data/str/val_files.txt", "tests/data/str/val_words.txt"}
UNTOUCHED = ["cnn", "cnn_in_time", "encoder", "attention", "decoder", "trainer", "adadelta", "runner"]


# ---- through the config loader ------------------------------------------------------------------------------------------
def sections(text):
    """name -> the section's text, header line included."""
    parts = re.split(r"(?m)^(?=\[[a-z_]+\]$)", text)
    return {re.match(r"\[([a-z_]+)\]", p).group(1): p for p in parts if p.startswith("[")}


def with_numpy_images(root, n_train=None, n_val=None, seed=5):
    """tests/str.ini with its [image_reader] and dataset sections alone replaced: the image reader becomes the NumPy
    reader over archives written here (synthetic 32 x 256 x 1 images, one per name of the reference's file lists, the
    right part of each blank), the datasets name (shortened) copies of the reference's lists.  -> the INI's name."""
    rng = np.random.default_rng(seed)
    data = os.path.join(root, "tests", "data", "str")
    images = os.path.join(root, "tests", "data", "str_numpy")
    os.makedirs(images, exist_ok=True)
    for split, count in (("train", n_train), ("val", n_val)):
        names = open(os.path.join(data, split + "_files.txt")).read().split("\n")
        words = open(os.path.join(data, split + "_words.txt")).read().split("\n")
        names, words = [n for n in names if n][:count], [w for w in words if w][:count]
        assert len(names) == len(words) and names
        for name in names:
            image = rng.uniform(1.0, 255.0, (32, 256, 1)).astype(np.float32)
            image[:, int(rng.integers(100, 256)):] = 0.0
            os.makedirs(os.path.dirname(os.path.join(images, name)), exist_ok=True)
            np.savez(os.path.join(images, name + ".npz"), image)
        for kind, lines in (("files", names), ("words", words)):
            with open(os.path.join(images, "{}_{}.txt".format(split, kind)), "w") as handle:
                handle.write("\n".join(lines) + "\n")
    text = open(os.path.join(root, "tests", "str.ini")).read()
    before = sections(text)
    edited, n = re.subn(r"\[image_reader\]\n(?:[^\[\n][^\n]*\n)+",
                        '[image_reader]\nclass=readers.numpy_reader.from_file_list\nprefix="{}"\n'
                        'shape=[32, 256, 1]\nsuffix=".npz"\n'.format(images), text)
    assert n == 1
    for split in ("train", "val"):
        for kind in ("files", "words"):
            old = "tests/data/str/{}_{}.txt".format(split, kind)
            assert old in edited
            edited = edited.replace(old, "tests/data/str_numpy/{}_{}.txt".format(split, kind))
    after = sections(edited)
    assert set(after) == set(before)
    changed = {k for k in before if before[k] != after[k]}
    assert changed == {"image_reader", "train_data", "val_data", "val_data_no_target"}
    assert all(before[k] == after[k] for k in UNTOUCHED)
    with open(os.path.join(root, "tests", "str_numpy.ini"), "w") as handle:
        handle.write(edited)
    return "str_numpy"


@pytest.fixture(scope="module")
def str_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("str_tests")
    with tarfile.open(M.BUNDLE) as tar:
        tar.extractall(root)
    return str(root)


BN = ("gamma", "beta", "moving_mean", "moving_variance")


def str_ini_cnn_variables():
    """The [cnn] section's variables: 32 x 256 x 1 images, C 3 valid 4, M 2 2, R 3 12, A 2 1 with batch norm."""
    want = {}

    def conv(scope, k, cin, cout):
        want[scope + "/conv2d/kernel"], want[scope + "/conv2d/bias"] = (k, k, cin, cout), (cout,)

    def bn(scope, c):
        for leaf in BN:
            want[scope + "/batch_normalization/" + leaf] = (c,)
    conv("cnn/convolutions/layer_0_convolution", 3, 1, 4)
    bn("cnn/convolutions/layer_0_convolution", 4)
    block = "cnn/convolutions/layer_2_resnet_block"
    conv(block + "/project_input", 1, 4, 12)
    bn(block + "/project_input", 12)
    bn(block + "/conv_a", 4)
    conv(block + "/conv_a", 3, 4, 12)
    bn(block + "/conv_b", 12)
    conv(block + "/conv_b", 3, 12, 12)
    return want


def test_str_ini_builds_with_numpy_images(str_root):
    """Fails on a tree without the feature with SymbolNotShipped (encoders.cnn_encoder does not exist there)."""
    from .test_reference_inis import load_verbatim
    from neuralmonkey_amd.attention import Attention
    from neuralmonkey_amd.decoders import Decoder
    from neuralmonkey_amd.encoders import RecurrentEncoder
    from neuralmonkey_amd.encoders.cnn_encoder import CNNEncoder, CNNTemporalView
    from neuralmonkey_amd.optimizers import AdadeltaOptimizer
    from neuralmonkey_amd.runners import GreedyRunner
    model = load_verbatim(str_root, with_numpy_images(str_root), device="cpu")
    runner, = model.runners
    dec = runner.decoder
    assert isinstance(runner, GreedyRunner) and isinstance(dec, Decoder) and runner.output_series == "target_chars"
    enc, = dec.encoders
    att, = dec.attentions
    assert type(enc) is RecurrentEncoder and isinstance(att, Attention) and att.encoder is enc
    view = enc.input_sequence
    assert type(view) is CNNTemporalView and view.name == "cnn_in_time"
    cnn = view._cnn                                                       # pylint: disable=protected-access
    assert type(cnn) is CNNEncoder and cnn.name == "cnn" and cnn.batch_normalize is True
    assert cnn.convolutions == [("C", 3, 1, "valid", 4), ("M", 2, 2, "same"), ("R", 3, 12), ("A", 2, 1, "same")]
    assert (cnn.image_height, cnn.image_width, cnn.pixel_dim, cnn.dropout_keep_prob) == (32, 256, 1, 0.5)
    assert cnn.spatial_shape == (14, 126, 12) and view.dimension == 14 * 12 and view.output_size == 12
    assert "_cnn" in view.dependencies and cnn in view.get_dependencies()[0] and cnn in enc.get_dependencies()[1]
    assert cnn.graph_safe_training(True) is False
    trainer, = model.trainers
    assert isinstance(trainer.optimizer, AdadeltaOptimizer) and trainer.objectives[0].decoder is dec
    store = model.tf_manager.sessions[0].store
    mine = {n: tuple(store[n].shape) for n in store.names() if n.startswith("cnn")}
    assert mine == str_ini_cnn_variables()
    frozen = sorted(n for n in mine if n not in store.trainable_names())
    assert frozen == sorted(n for n in mine if n.endswith(("moving_mean", "moving_variance"))) and len(frozen) == 8
    assert not any(n.startswith("cnn_in_time/") for n in store.names())
    gates = [tuple(store[n].shape) for n in store.names() if n.startswith("encoder/") and n.endswith("gates/kernel")]
    assert gates and all(shape == (14 * 12 + 256, 512) for shape in gates)       # the GRU reads the map's columns
    batch = next(iter(model.train_dataset.batches()))
    fd = cnn.feed_dict(batch, train=True)
    images = fd[cnn.image_input]
    assert images.dtype == np.float32 and images.shape == (len(batch), 32, 256, 1) and 0.9 < images.max() <= 1.0
    assert np.array_equal(images, (np.array(list(batch.get_series("images"))) / 255.0).astype(np.float32))


def test_archive_members_are_the_references_bytes(str_root):
    with tarfile.open(M.BUNDLE) as tar:
        names = [m.name for m in tar.getmembers()]
    assert set(names) == MEMBERS and len(names) == 6
    assert os.path.getsize(M.BUNDLE) < 16 * 1024
    if os.path.isdir(REF):
        for rel in names:
            with open(os.path.join(REF, rel), "rb") as a, open(os.path.join(str_root, rel), "rb") as b:
                assert a.read() == b.read(), rel


# ---- signatures and argument checks --------------------------------------------------------------------------------------
def test_constructor_parameters_are_the_references():
    from .test_reference_signatures import product_parameters, read_reference_parameters
    path = "encoders/cnn_encoder.py"
    with open(M.LISTS, encoding="utf-8") as handle:
        lists = json.load(handle)
    assert list(lists) == [path] and sorted(lists[path]) == ["CNNEncoder", "CNNTemporalView"]
    for name in lists[path]:
        want = [tuple(p) for p in lists[path][name]]
        if os.path.isdir(REF):
            assert read_reference_parameters(path, name) == want
        assert product_parameters(path, name) == want
    assert [p[0] for p in lists[path]["CNNEncoder"]] == [
        "name", "data_id", "convolutions", "image_height", "image_width", "pixel_dim", "fully_connected",
        "batch_normalize", "dropout_keep_prob", "reuse", "save_checkpoint", "load_checkpoint", "initializers"]
    assert [p[0] for p in lists[path]["CNNTemporalView"]] == ["name", "cnn"]


def make(convolutions, name="cnn", **kw):
    from neuralmonkey_amd.encoders.cnn_encoder import CNNEncoder
    args = dict(data_id="images", image_height=12, image_width=20, pixel_dim=1)
    args.update(kw)
    return CNNEncoder(name=name, convolutions=convolutions, **args)


def test_constructor_defaults_and_refusals_use_the_references_words():
    import inspect
    from neuralmonkey_amd.encoders.cnn_encoder import CNNEncoder, CNNTemporalView
    from neuralmonkey_amd.model.stateful import SpatialStatefulWithOutput, TemporalStatefulWithOutput
    from neuralmonkey_amd.runtime import reset_registry
    reset_registry()
    defaults = {k: p.default for k, p in inspect.signature(CNNEncoder.__init__).parameters.items()}
    assert (defaults["fully_connected"], defaults["batch_normalize"], defaults["dropout_keep_prob"]) == (None, False, 0.5)
    assert isinstance(make([("C", 3, 1, "same", 4), ("M", 2, 2, "same")], name="a"), SpatialStatefulWithOutput)
    # the convolution ignores its stride and the mask's pooling does not: the shapes part
    with pytest.raises(ValueError, match=r"after layer 0 .* the states are 12 x 20 and the mask is 6 x 10"):
        make([("C", 3, 2, "same", 4)], name="b").spatial_shape  # pylint: disable=expression-not-assigned
    messages = [
        ([("R", 3, 4)], {}, "Using ResNet blocks requires batch normalization to be turned on."),
        ([("X", 3, 4)], {}, "Unknown type of convoutional layer #1: 'X'"),
        ([("C", 3, 1, "full", 4)], {}, "Padding must be 'same' or 'valid', was 'full' in layer 1."),
        ([("C", 3, 1, "valid", 4), ("M", 2, 2, "full")], {}, "Padding must be 'same' or 'valid', was 'full' in layer 2."),
        ([("C", 3, 1, "valid")], {}, 'Specification of a convolutional layer (number 0 in config) needs to have 5 '
                                     'members: "C", kernel size, stride, padding, output channels, was '
                                     "('C', 3, 1, 'valid')"),
        ([("M", 2, 2)], {}, 'Specification of a max-pooling layer (number 0 in config) needs to have 3 members: "M", '
                            "pool size, stride, padding, was ('M', 2, 2)"),
        ([("R", 3, 4, "same")], dict(batch_normalize=True), 'Specification of a residual block (number 0 in config) needs '
                                                            'to have 3 members: "R", kernel size, channels; was '
                                                            "('R', 3, 4, 'same')"),
    ]
    for i, (convs, kw, text) in enumerate(messages):
        with pytest.raises(ValueError) as info:
            make(convs, name="bad{}".format(i), **kw)
        assert str(info.value) == text
    with pytest.raises(TypeError):
        make([("C", 3, 1, "valid", 4)], name="t1", image_height="12")
    with pytest.raises(TypeError):
        CNNTemporalView("view", "cnn")
    two = make([("C", 3, 1, "valid", 4), ("M", 2, 2, "same")], name="c")
    view = CNNTemporalView("view", two)
    assert isinstance(view, TemporalStatefulWithOutput) and two.spatial_shape == (5, 9, 4)
    assert (view.dimension, view.output_size, two.dimension, two.output_size) == (20, 4, 4, 4)
    assert make([("C", 3, 1, "valid", 4)], name="d", fully_connected=[9, 5]).output_size == 5
    if os.path.isdir(REF):                                      # the messages are the reference's own text
        text = open(os.path.join(REF, "neuralmonkey/encoders/cnn_encoder.py")).read()
        text = re.sub(r"[\"']\s*\n\s*[\"']", "", text)
        for message in ("Using ResNet blocks requires batch normalization to be turned on.",
                        "Unknown type of convoutional layer #{}: '{}'",
                        "Padding must be 'same' or 'valid', was '{}' in layer {}.",
                        "Specification of a convolutional layer (number {} in config) needs to have 5 members: ",
                        "Specification of a residual block (number {} in config) needs to have 3 members: ",
                        "Specification of a max-pooling layer (number {} in config) needs to have 3 members: "):
            assert message.replace("'", "").replace('"', "") in text.replace("'", "").replace('"', ""), message


# ---- variables -------------------------------------------------------------------------------------------------------------
def declared(parts):
    from neuralmonkey_amd.variables import VariableStore
    store = VariableStore("cpu", seed=3)
    for part in parts:
        part.declare_variables(store)
    return store


def recorded_variables(z):
    return {str(n): tuple(json.loads(str(s))) for n, s in zip(z["out/variable_names"], z["out/variable_shapes"])}


@pytest.mark.parametrize("case", M.ALL_CASES)
def test_declared_variables_are_the_ones_the_reference_created(case):
    z, cfg, params = M.load_fixture(case)
    want = recorded_variables(z)
    assert want == {n: tuple(v.shape) for n, v in params.items()}
    m = M.build_parts(cfg)
    store = declared(m["feedables"])
    mine = {n: s.shape for n, s in store.specs.items()}
    assert mine == want
    frozen = sorted(n for n, s in store.specs.items() if not s.trainable)
    assert frozen == sorted(str(n) for n in z["out/non_trainable"])
    assert all(n.endswith(("moving_mean", "moving_variance")) for n in frozen)
    assert bool(frozen) == cfg["batch_normalize"]
    assert [n for n in store.names() if n.startswith("cnn/")] == [n for n in z["out/variable_names"]
                                                                 if str(n).startswith("cnn/")]      # creation order


def test_initializers_are_tensorflows():
    """Kernels: glorot uniform with the receptive field in the fans; biases, beta and the moving mean 0; gamma and the
    moving variance 1."""
    from neuralmonkey_amd.runtime import reset_registry
    reset_registry()
    cnn = make([("C", 3, 1, "valid", 32), ("R", 3, 48)], batch_normalize=True, pixel_dim=16, fully_connected=[7])
    store = declared([cnn])
    store.finalize()
    v = {n: store[n].numpy() for n in store.names()}
    for name, (k, cin, cout) in (("cnn/convolutions/layer_0_convolution/conv2d/kernel", (3, 16, 32)),
                                 ("cnn/convolutions/layer_1_resnet_block/project_input/conv2d/kernel", (1, 32, 48)),
                                 ("cnn/convolutions/layer_1_resnet_block/conv_b/conv2d/kernel", (3, 48, 48))):
        lim = np.sqrt(6.0 / (k * k * (cin + cout)))
        assert v[name].shape == (k, k, cin, cout)
        assert 0.9 * lim < np.abs(v[name]).max() <= lim and abs(v[name].std() - lim / np.sqrt(3.0)) < 0.1 * lim, name
    for name, val in v.items():
        if name.endswith(("bias", "beta", "moving_mean")):
            assert not val.any(), name
        if name.endswith(("gamma", "moving_variance")):
            assert (val == 1.0).all(), name
    assert v["cnn/mlp/mlp_layer_0/kernel"].shape == (10 * 18 * 48, 7)


# ---- the fixtures ----------------------------------------------------------------------------------------------------------
def test_fixture_directory_holds_the_issues_cases():
    have = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(M.FIX, "*.npz")))
    assert have == sorted(M.ALL_CASES)
    str_stack = [["C", 3, 1, "valid", 4], ["M", 2, 2, "same"], ["R", 3, 12], ["A", 2, 1, "same"]]
    for case in M.ALL_CASES:
        z, cfg, params = M.load_fixture(case)
        assert os.path.getsize(os.path.join(M.FIX, case + ".npz")) < 64 * 1024
        images = z["in/images"]
        assert images.shape == (3, cfg["height"], cfg["width"], cfg["pixel_dim"]) and images.max() > 200
        third = cfg["width"] - cfg["width"] // 3
        assert not images[1, :, third:].any() and images[1, :, :third].all() and images[0].all() and images[2].all()
        for prefix, train in M.passes(case, cfg):
            got = M.recorded(z, prefix)
            assert {"spatial_states", "spatial_mask", "output", "image_mask"} <= set(got)
            assert 0 < got["spatial_mask"].sum() < got["spatial_mask"].size         # the mask is not all ones
            assert any(k.startswith("stats/") for k in got) == (train and cfg["batch_normalize"])
    assert M.load_fixture("cnn_str_stack")[1]["convolutions"] == str_stack
    assert M.load_fixture("cnn_fc")[1]["fully_connected"] == [9, 5]
    same = M.load_fixture("cnn_resnet_same_channels")[1]["convolutions"]
    assert same[0][4] == same[1][2] and same[1][0] == "R"                          # no projection
    assert not any("project_input" in n for n in M.load_fixture("cnn_resnet_same_channels")[2])
    plain = M.load_fixture("cnn_plain")[1]["convolutions"]
    assert [s[0] for s in plain] == ["C", "M", "C", "A"] and plain[2][1] == 2 and plain[2][3] == "same"
    for case in M.FD_CASES:
        z, cfg, params = M.load_fixture(case)
        names = [str(n) for n in z["fd/names"]]
        frozen = {str(n) for n in z["out/non_trainable"]}
        assert set(names) == set(params) - frozen and cfg["train_mode"] is True
        h = float(z["fd/h"])
        assert all(names.count(n) == min(3, params[n].size) for n in set(names))
        assert float(z["fd/relu_margin"]) > 100 * h and float(z["fd/max_margin"]) > 100 * h


@pytest.mark.parametrize("case", M.ALL_CASES)
def test_numpy_restatement_reproduces_the_reference(case):
    z, cfg, params = M.load_fixture(case)
    for prefix, train in M.passes(case, cfg):
        want = M.recorded(z, prefix)
        got = M.restate(cfg, params, z["in/images"], train)
        mine = [k for k in want if k in got]
        others = sorted(set(want) - set(got))
        assert all(k in ("enc_states", "enc_output", "pool_output", "decoded_logits", "cost") for k in others), others
        assert {"spatial_states", "spatial_mask", "output", "image_mask"} <= set(mine)
        if cfg["head"] == "temporal":
            assert {"temporal_states", "temporal_mask"} <= set(mine)
        for key in mine:
            assert got[key].shape == want[key].shape, key
            if key.endswith("mask"):
                assert np.array_equal(got[key], want[key]), key
            else:
                assert np.abs(got[key] - want[key]).max() <= 1e-9, (key, np.abs(got[key] - want[key]).max())


def test_numpy_window_takes_the_first_maximum_and_tensorflows_same_padding():
    x = np.zeros((1, 3, 3, 1))
    x[0, :, :, 0] = [[1, 5, 5], [5, 2, 5], [0, 0, 0]]
    out, where = M.np_window2d(x, (2, 2), (1, 1), "valid", "max")
    assert out[0, :, :, 0].tolist() == [[5, 5], [5, 5]] and where[0, :, :, 0].tolist() == [[1, 1], [3, 5]]
    out, _ = M.np_window2d(x, (2, 2), (2, 2), "same", "max")                  # 3 -> 2 windows, the pad after the map
    assert out[0, :, :, 0].tolist() == [[5, 5], [0, 0]]
    assert M.np_pad(5, 2, 1, "same") == (5, 0) and M.np_pad(5, 3, 1, "same") == (5, 1) and M.np_pad(5, 4, 1, "same") == (5, 1)
    assert M.np_pad(15, 2, 2, "valid") == (7, 0) and M.np_pad(15, 2, 2, "same") == (8, 0)


# ---- checkpoints ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["tf", "npz"])
def test_checkpoint_round_trip_carries_the_moving_statistics(tmp_path, fmt):
    """Moving statistics are saved and restored; being non-trainable they have no optimizer slots, and a checkpoint
    without slots for them still restores the slots of everything else."""
    from neuralmonkey_amd import tf_bundle
    from neuralmonkey_amd.variables import VariableStore
    z, cfg, params = M.load_fixture("cnn_str_stack")

    def store_of(seed):
        store = VariableStore("cpu", seed=seed)
        M.build_parts(cfg)["cnn"].declare_variables(store)
        store.finalize()
        return store
    a = store_of(1)
    a.load_state_dict({k: v.astype(np.float32) for k, v in params.items()})
    m, v = a.ensure_adam()
    m.copy_(__import__("torch").arange(a.total, dtype=__import__("torch").float32))
    v.fill_(0.25)
    path = str(tmp_path / ("variables.data" if fmt == "tf" else "variables.npz"))
    a.save(path, fmt=fmt, global_step=7)
    if fmt == "tf":
        keys = set(tf_bundle.read_bundle(path))
    else:
        keys = {k.replace("|", "/") for k in np.load(path).files}
    frozen = [n for n, s in a.specs.items() if not s.trainable]
    assert len(frozen) == 8
    for name, spec in a.specs.items():
        assert name in keys
        assert (name + "/Adam" in keys) == spec.trainable and (name + "/Adam_1" in keys) == spec.trainable, name
    b = store_of(2)
    assert b.load(path)["global_step"] == 7
    for name in a.names():
        assert np.array_equal(a[name].numpy(), b[name].numpy()), name
    for name in frozen:
        assert np.array_equal(b[name].numpy(), params[name].astype(np.float32).reshape(b[name].shape))
    assert b.adam_m is not None
    for name, spec in a.specs.items():
        if spec.trainable:
            sl = slice(spec.offset, spec.offset + spec.size)
            assert np.array_equal(a.adam_m[sl].numpy(), b.adam_m[sl].numpy()) and (b.adam_v[sl] == 0.25).all()


# ---- the sixth binding table ----------------------------------------------------------------------------------------------
def image_header_symbols():
    text = open(os.path.join(ROOT, "include", "nmhip_image.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nm_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


def test_image_header_matches_its_binding_table(lib):
    from neuralmonkey_amd import _lib
    from .test_abi import header_symbols
    from .test_convs2s_host import convs2s_header_symbols
    from .test_ctc_host import ctc_header_symbols
    from .test_labeler_host import label_header_symbols
    from .test_pool_host import pool_header_symbols
    mine = image_header_symbols()
    assert mine == set(_lib.IMAGE_SIGNATURES) and len(mine) == 8
    for other in (_lib.SIGNATURES, _lib.CTC_SIGNATURES, _lib.LABEL_SIGNATURES, _lib.POOL_SIGNATURES,
                  _lib.CONVS2S_SIGNATURES):
        assert not mine & set(other)
    for theirs in (header_symbols, ctc_header_symbols, label_header_symbols, pool_header_symbols, convs2s_header_symbols):
        assert not mine & theirs()
    for name, (res, args) in _lib.IMAGE_SIGNATURES.items():
        fn = getattr(lib, name)                                          # exported, and bound by load()
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    header = open(os.path.join(ROOT, "include", "nmhip_image.h")).read()
    for cited in ("cnn_encoder.py:231", ":265", ":273", ":280", "cnn_encoder.py:107", "cnn_encoder.py:318-319", ":238",
                  ":187", "cnn_encoder.py:340-344"):
        assert cited in header, cited                                    # the lines it replaces


def test_image_entry_points_refuse_before_any_launch(lib):
    """Host buffers and a null stream: a call that got as far as a launch would fault or fail differently."""
    buf = (ctypes.c_float * 65536)()
    other = (ctypes.c_float * 65536)()
    third = (ctypes.c_float * 65536)()
    ints = (ctypes.c_int32 * 65536)()

    def check(fn, cases):
        for kwargs, text in cases:
            assert fn(**kwargs) < 0 and lib.nm_last_error() == text, (kwargs, lib.nm_last_error())

    def fwd(x=buf, ldx=8, b=2, h=5, w=6, cin=8, filt=third, k=3, cout=4, pad=0, bias=third, y=other, ldy=4, algo=0):
        return lib.nm_conv2d_fwd(None, x, ldx, b, h, w, cin, filt, k, cout, pad, bias, y, ldy, algo)
    check(fwd, (
        (dict(b=0), b"nm_conv2d_fwd: bad sizes B 0, H 5, W 6, Cin 8, Cout 4, k 3"),
        (dict(cout=0), b"nm_conv2d_fwd: bad sizes B 2, H 5, W 6, Cin 8, Cout 0, k 3"),
        (dict(k=0), b"nm_conv2d_fwd: bad sizes B 2, H 5, W 6, Cin 8, Cout 4, k 0"),
        (dict(pad=2), b"nm_conv2d_fwd: padding 2 (0 VALID, 1 SAME)"),
        (dict(h=2), b"nm_conv2d_fwd: VALID padding with a 2 x 6 map below the 3 x 3 filter"),
        (dict(w=2), b"nm_conv2d_fwd: VALID padding with a 5 x 2 map below the 3 x 3 filter"),
        (dict(b=1 << 20, h=1 << 8, w=1 << 8), b"nm_conv2d_fwd: a map or the filter holds more than 2^31 - 1 elements"),
        (dict(x=None), b"nm_conv2d_fwd: null pointer"), (dict(filt=None), b"nm_conv2d_fwd: null pointer"),
        (dict(bias=None), b"nm_conv2d_fwd: null pointer"), (dict(y=None), b"nm_conv2d_fwd: null pointer"),
        (dict(ldx=7), b"nm_conv2d_fwd: ldx 7 below Cin 8"), (dict(ldy=3), b"nm_conv2d_fwd: ldy 3 below Cout 4"),
        (dict(y=buf), b"nm_conv2d_fwd: y overlapping x"),
        (dict(y=ctypes.byref(buf, 4 * 100)), b"nm_conv2d_fwd: y overlapping x"),
        (dict(algo=3), b"nm_conv2d_fwd: algo 3 (0 auto, 1 mfma, 2 scalar)"),
        (dict(algo=-1), b"nm_conv2d_fwd: algo -1 (0 auto, 1 mfma, 2 scalar)"),
        (dict(algo=1, k=8, h=9, w=9), b"nm_conv2d_fwd: the MFMA kernel takes k <= 7, not 8")))

    one = (3 * 3 * 8 * 4 + 4) * 4                                      # 2*3*4 = 24 positions: one slice
    assert lib.nm_conv2d_workspace_bytes(2, 5, 6, 8, 3, 4, 0) == one
    assert lib.nm_conv2d_workspace_bytes(2, 5, 6, 8, 3, 4, 1) == one   # 60 positions: still one
    assert lib.nm_conv2d_workspace_bytes(4, 32, 256, 8, 3, 4, 1) == 256 * one
    for bad in ((0, 5, 6, 8, 3, 4, 0), (2, 2, 6, 8, 3, 4, 0), (2, 5, 6, 8, 3, 4, 2), (1 << 31, 5, 6, 8, 3, 4, 0)):
        assert lib.nm_conv2d_workspace_bytes(*bad) == 0

    def bwd(x=buf, ldx=8, b=2, h=5, w=6, cin=8, filt=third, k=3, cout=4, pad=0, dy=other, lddy=4, dx=None, lddx=8, acc=0,
            dw=None, db=None, accp=0, ws=None, ws_bytes=0, algo=0):
        dx = ctypes.byref(other, 4 * 4096) if dx is None else dx
        return lib.nm_conv2d_bwd(None, x, ldx, b, h, w, cin, filt, k, cout, pad, dy, lddy, dx, lddx, acc, dw, db, accp, ws,
                                 ws_bytes, algo)
    check(bwd, (
        (dict(cin=0), b"nm_conv2d_bwd: bad sizes B 2, H 5, W 6, Cin 0, Cout 4, k 3"),
        (dict(h=2), b"nm_conv2d_bwd: VALID padding with a 2 x 6 map below the 3 x 3 filter"),
        (dict(x=None), b"nm_conv2d_bwd: null pointer"), (dict(filt=None), b"nm_conv2d_bwd: null pointer"),
        (dict(dy=None), b"nm_conv2d_bwd: null pointer"),
        (dict(ldx=7), b"nm_conv2d_bwd: ldx 7 below Cin 8"), (dict(lddy=3), b"nm_conv2d_bwd: lddy 3 below Cout 4"),
        (dict(lddx=7), b"nm_conv2d_bwd: lddx 7 below Cin 8"),
        (dict(dx=other), b"nm_conv2d_bwd: dx overlapping dy"),
        (dict(dx=ctypes.byref(other, 4 * 40)), b"nm_conv2d_bwd: dx overlapping dy"),
        (dict(algo=4), b"nm_conv2d_bwd: algo 4 (0 auto, 1 mfma, 2 scalar)"),
        (dict(algo=1, k=8, h=9, w=9), b"nm_conv2d_bwd: the MFMA kernels take k <= 7, not 8"),
        (dict(dw=third), b"nm_conv2d_bwd: the filter and bias gradients need a workspace"),
        (dict(db=third), b"nm_conv2d_bwd: the filter and bias gradients need a workspace"),
        (dict(dw=third, ws=ints, ws_bytes=one - 1),
         "nm_conv2d_bwd: workspace too small ({} < {} bytes)".format(one - 1, one).encode())))

    def bn(x=buf, ldx=8, rows=30, c=8, gamma=third, beta=third, eps=1e-3, mom=0.99, train=1, relu=1, mm=None, mv=None,
           bm=other, bv=other, y=ctypes.byref(other, 4 * 4096), ldy=8):
        return lib.nm_bn2d_fwd(None, x, ldx, rows, c, gamma, beta, eps, mom, train, relu, mm, mv, bm, bv, y, ldy)
    check(bn, (
        (dict(rows=0), b"nm_bn2d_fwd: bad sizes rows 0, C 8"), (dict(c=0), b"nm_bn2d_fwd: bad sizes rows 30, C 0"),
        (dict(rows=1 << 30, c=4), b"nm_bn2d_fwd: rows * C = 4294967296 elements beyond 2^31 - 1"),
        (dict(x=None), b"nm_bn2d_fwd: null pointer"), (dict(gamma=None), b"nm_bn2d_fwd: null pointer"),
        (dict(beta=None), b"nm_bn2d_fwd: null pointer"), (dict(y=None), b"nm_bn2d_fwd: null pointer"),
        (dict(ldx=7), b"nm_bn2d_fwd: ldx 7 below C 8"), (dict(ldy=7), b"nm_bn2d_fwd: ldy 7 below C 8"),
        (dict(eps=0.0), b"nm_bn2d_fwd: eps 0 must be positive"),
        (dict(mom=1.5), b"nm_bn2d_fwd: momentum 1.5 outside [0, 1]"),
        (dict(mm=third), b"nm_bn2d_fwd: moving_mean and moving_var come together or not at all"),
        (dict(bm=None), b"nm_bn2d_fwd: training needs batch_mean and batch_var"),
        (dict(train=0), b"nm_bn2d_fwd: inference needs moving_mean and moving_var")))

    def bnb(x=buf, ldx=8, y=third, ldy=8, dy=other, lddy=8, rows=30, c=8, gamma=third, bm=third, bv=third, eps=1e-3, relu=1,
            dx=None, lddx=8, acc=0, dg=None, db=None, accp=0, sums=ctypes.byref(third, 4 * 4096)):
        dx = ctypes.byref(other, 4 * 4096) if dx is None else dx
        return lib.nm_bn2d_bwd(None, x, ldx, y, ldy, dy, lddy, rows, c, gamma, bm, bv, eps, relu, dx, lddx, acc, dg, db,
                               accp, sums)
    check(bnb, (
        (dict(rows=0), b"nm_bn2d_bwd: bad sizes rows 0, C 8"),
        (dict(x=None), b"nm_bn2d_bwd: null pointer"), (dict(dy=None), b"nm_bn2d_bwd: null pointer"),
        (dict(gamma=None), b"nm_bn2d_bwd: null pointer"), (dict(bm=None), b"nm_bn2d_bwd: null pointer"),
        (dict(bv=None), b"nm_bn2d_bwd: null pointer"), (dict(sums=None), b"nm_bn2d_bwd: null pointer"),
        (dict(y=None), b"nm_bn2d_bwd: the ReLU gate needs the saved output y"),
        (dict(ldx=7), b"nm_bn2d_bwd: ldx 7 below C 8"), (dict(ldy=7), b"nm_bn2d_bwd: ldy 7 below C 8"),
        (dict(lddy=7), b"nm_bn2d_bwd: lddy 7 below C 8"), (dict(lddx=7), b"nm_bn2d_bwd: lddx 7 below C 8"),
        (dict(dx=ctypes.byref(other, 4 * 40)), b"nm_bn2d_bwd: dx partially overlapping dy")))

    def win(x=buf, ldx=4, b=2, h=7, w=9, c=4, kh=3, kw=3, sh=2, sw=2, pad=0, mode=0, y=other, ldy=4, arg=None):
        return lib.nm_window2d_fwd(None, x, ldx, b, h, w, c, kh, kw, sh, sw, pad, mode, y, ldy, arg)
    check(win, (
        (dict(c=0), b"nm_window2d_fwd: bad sizes B 2, H 7, W 9, C 0"),
        (dict(kh=0), b"nm_window2d_fwd: bad window 0 x 3, stride 2 x 2"),
        (dict(sw=0), b"nm_window2d_fwd: bad window 3 x 3, stride 2 x 0"),
        (dict(pad=3), b"nm_window2d_fwd: padding 3 (0 VALID, 1 SAME)"),
        (dict(mode=2), b"nm_window2d_fwd: mode 2 (0 max, 1 average)"),
        (dict(kh=8), b"nm_window2d_fwd: VALID padding with a 7 x 9 map below the 8 x 3 window"),
        (dict(x=None), b"nm_window2d_fwd: null pointer"), (dict(y=None), b"nm_window2d_fwd: null pointer"),
        (dict(ldx=3), b"nm_window2d_fwd: ldx 3 below C 4"), (dict(ldy=3), b"nm_window2d_fwd: ldy 3 below C 4"),
        (dict(y=ctypes.byref(buf, 4 * 8)), b"nm_window2d_fwd: y overlapping x")))

    def winb(dy=other, lddy=4, arg=ints, b=2, h=7, w=9, c=4, kh=3, kw=3, sh=2, sw=2, pad=0, mode=0, dx=buf, lddx=4, acc=0):
        return lib.nm_window2d_bwd(None, dy, lddy, arg, b, h, w, c, kh, kw, sh, sw, pad, mode, dx, lddx, acc)
    check(winb, (
        (dict(h=0), b"nm_window2d_bwd: bad sizes B 2, H 0, W 9, C 4"),
        (dict(mode=-1), b"nm_window2d_bwd: mode -1 (0 max, 1 average)"),
        (dict(dy=None), b"nm_window2d_bwd: null pointer"), (dict(dx=None), b"nm_window2d_bwd: null pointer"),
        (dict(arg=None), b"nm_window2d_bwd: the maximum's gradient needs argmax"),
        (dict(lddy=3), b"nm_window2d_bwd: lddy 3 below C 4"), (dict(lddx=3), b"nm_window2d_bwd: lddx 3 below C 4"),
        (dict(dx=ctypes.byref(other, 4 * 8)), b"nm_window2d_bwd: dx overlapping dy")))

    def cols(src=buf, dst=other, b=2, h=3, w=5, c=4, inv=0):
        return lib.nm_map_columns(None, src, dst, b, h, w, c, inv)
    check(cols, (
        (dict(w=0), b"nm_map_columns: bad sizes B 2, H 3, W 0, C 4"),
        (dict(b=1 << 20, h=1 << 10, w=1 << 10), b"nm_map_columns: a map holds more than 2^31 - 1 elements"),
        (dict(src=None), b"nm_map_columns: null pointer"), (dict(dst=None), b"nm_map_columns: null pointer"),
        (dict(dst=ctypes.byref(buf, 4 * 8)), b"nm_map_columns: dst overlapping src")))


def test_kernels_of_the_image_stack_do_not_spill(lib):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_resources
    finally:
        sys.path.pop(0)
    everything = kernel_resources()
    mine = {k: v for k, v in everything.items() if "img2d_" in k}
    assert len(mine) == 12, sorted(mine)
    assert all(v["scratch"] == 0 for v in mine.values()), {k: v["scratch"] for k, v in mine.items()}
    src = open(os.path.join(ROOT, "neuralmonkey_amd", "csrc", "nm_image.hip")).read()
    names = re.findall(r"__global__.*?void\s+(\w+)\s*\(", src, flags=re.S)
    assert len(names) == 12 and all(n.startswith("img2d_") for n in names), names
    # the substrings by which other files' no-spill tests count their own kernels
    for taken in ("pool_fwd_kernel", "pool_bwd_kernel", "time_softmax_", "sqerr_rows_kernel", "ctc_", "convs2s_",
                  "label_rows_kernel", "label_from_stats_kernel", "gru_cluster_", "nematus_cluster_", "gemm_tiled"):
        assert not any(taken in k for k in mine), taken
    mfma, = [v for k, v in mine.items() if "img2d_conv_mfma" in k]
    assert mfma["lds"] == (16 * 136 + 7 * 16 * 64) * 4
