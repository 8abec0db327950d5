"""The ImageNet encoder without a GPU: the constructor against the reference's source, the layer tables of VGG-16 and
VGG-19 (endpoints, variables, parameter counts), the reference's tests/captioning.ini through the config loader (see
tests/imagenet_models.py for the one value that has to change, and why), refusals with the reference's words, and the
binding table of include/nmhip_vgg.h with its argument checks on the CPU-built library."""
import ast
import ctypes
import inspect
import json
import os
import re
import tarfile

import numpy as np
import pytest

from . import imagenet_models as M
from . import imagenet_ref as ref
from .test_reference_inis import REF, load_verbatim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = "encoders/imagenet_encoder.py"
LISTS = os.path.join(M.GOLDEN, "imagenet_signatures.json")
CONV5_3 = {"vgg_16": 14714688, "vgg_19": 20024384}
WHOLE = {"vgg_16": 138357544, "vgg_19": 143667240}


def make(name="imagenet", network_type="vgg_16", **kw):
    from neuralmonkey_amd.encoders.imagenet_encoder import ImageNet
    args = dict(data_id="images", slim_models_path="nowhere/research/slim")
    args.update(kw)
    return ImageNet(name=name, network_type=network_type, **args)


# ---- the public surface ----------------------------------------------------------------------------------------------------
def test_reference_class_path_resolves():
    """Fails on a tree without the feature with SymbolNotShipped."""
    from neuralmonkey_amd.config.builder import resolve_symbol
    from neuralmonkey_amd.encoders import imagenet_encoder as E
    assert resolve_symbol("encoders.imagenet_encoder.ImageNet") is E.ImageNet
    assert resolve_symbol("neuralmonkey.encoders.imagenet_encoder.ImageNet") is E.ImageNet


def test_constructor_parameters_are_the_references():
    from neuralmonkey_amd.encoders.imagenet_encoder import ImageNet
    from .test_reference_signatures import product_parameters, read_reference_parameters
    with open(LISTS, encoding="utf-8") as handle:
        lists = json.load(handle)
    assert list(lists) == [PATH] and list(lists[PATH]) == ["ImageNet"]
    want = [tuple(p) for p in lists[PATH]["ImageNet"]]
    if os.path.isdir(REF):
        assert read_reference_parameters(PATH, "ImageNet") == want
    assert product_parameters(PATH, "ImageNet") == want
    assert [p[0] for p in want] == ["name", "data_id", "network_type", "slim_models_path", "load_checkpoint",
                                    "spatial_layer", "encoded_layer", "initializers"]
    defaults = {k: p.default for k, p in inspect.signature(ImageNet.__init__).parameters.items() if k != "self"}
    assert [defaults[k] for k in ("load_checkpoint", "spatial_layer", "encoded_layer", "initializers")] == [None] * 4


def test_supported_networks_are_the_references_keys():
    from neuralmonkey_amd.encoders import imagenet_encoder as E
    keys = ["alexnet_v2", "vgg_16", "vgg_19", "resnet_v2_50", "resnet_v2_101", "resnet_v2_152"]
    assert list(E.SUPPORTED_NETWORKS) == keys
    if os.path.isdir(REF):
        tree = ast.parse(open(os.path.join(REF, "neuralmonkey", PATH)).read())
        table, = [n.value for n in tree.body if isinstance(n, ast.Assign) and n.targets[0].id == "SUPPORTED_NETWORKS"]
        assert [k.value for k in table.keys] == keys


# ---- the layer tables -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["vgg_16", "vgg_19"])
def test_layer_table_endpoints_variables_and_parameter_counts(net):
    from neuralmonkey_amd.encoders import imagenet_encoder as E
    layers = E.layer_table(net)
    blocks = {"vgg_16": (2, 2, 3, 3, 3), "vgg_19": (2, 2, 4, 4, 4)}[net]
    widths = (64, 128, 256, 512, 512)
    names, shapes, cin, size = [], {}, 3, 224
    sizes = {}
    for n, (count, cout) in enumerate(zip(blocks, widths), start=1):
        for m in range(1, count + 1):
            scope = "{}/conv{}/conv{}_{}".format(net, n, n, m)
            names.append(scope)
            shapes[scope + "/weights"], shapes[scope + "/biases"] = (3, 3, cin, cout), (cout,)
            sizes[scope] = (size, size, cout)
            cin = cout
        size //= 2
        names.append("{}/pool{}".format(net, n))
        sizes[names[-1]] = (size, size, cout)
    for scope, k, cout in ((net + "/fc6", 7, 4096), (net + "/fc7", 1, 4096), (net + "/fc8", 1, 1000)):
        names.append(scope)
        shapes[scope + "/weights"], shapes[scope + "/biases"] = (k, k, cin, cout), (cout,)
        sizes[scope] = (1, 1, cout) if scope != net + "/fc8" else (cout,)
        cin = cout
    assert [layer.endpoint for layer in layers] == names                  # in order
    assert [layer.endpoint for layer in layers] == [row[0] for row in ref.layers(net)]
    assert {layer.endpoint: layer.out_shape for layer in layers} == sizes
    declared = [(name, shape) for layer in layers for name, shape in layer.variables]
    assert dict(declared) == shapes and len(declared) == len(shapes)
    assert [name for name, _ in declared] == [n + leaf for n in names if "pool" not in n for leaf in ("/weights", "/biases")]
    last_conv = "{}/conv5/conv5_{}".format(net, blocks[4])
    assert E.parameter_count(net, last_conv) == CONV5_3[net]
    assert E.parameter_count(net) == WHOLE[net]                           # from the table: nothing is allocated
    assert sum(int(np.prod(s)) for s in shapes.values()) == WHOLE[net]
    for layer in layers:
        assert (layer.kind == "conv") == ("/conv" in layer.endpoint) and (layer.kind == "pool") == ("/pool" in layer.endpoint)
        assert layer.relu == (layer.kind != "pool" and not layer.endpoint.endswith("fc8"))


def test_only_the_layers_in_use_are_declared_under_slims_names_and_frozen(monkeypatch):
    from neuralmonkey_amd.runtime import reset_registry
    from neuralmonkey_amd.variables import VariableStore
    reset_registry()
    M.narrow(monkeypatch)
    a = make("first", spatial_layer="vgg_16/conv3/conv3_2")
    b = make("second", spatial_layer="vgg_16/conv2/conv2_1", encoded_layer="vgg_16/fc7")
    c = make("third", network_type="vgg_19", spatial_layer="vgg_19/pool5")
    assert (a.scope, b.scope, c.scope) == ("vgg_16", "vgg_16", "vgg_19") and a.name == "first"
    assert (a.dimension, a.output_size, b.dimension, b.output_size, c.dimension) == (16, 16, 8, 64, 32)
    store = VariableStore("cpu", seed=3)
    a.declare_variables(store)
    only_a = store.names()
    assert only_a[0] == "vgg_16/conv1/conv1_1/weights" and only_a[-1] == "vgg_16/conv3/conv3_2/biases"
    assert len(only_a) == 2 * 6 and not any(n.startswith("first") for n in only_a)
    for part in (b, c):
        part.declare_variables(store)                                    # a and b share vgg_16/...
    names = store.names()
    assert "vgg_16/fc7/weights" in names and "vgg_16/fc8/weights" not in names
    assert "vgg_19/conv5/conv5_4/biases" in names and "vgg_19/fc6/weights" not in names
    assert store.trainable_names() == []
    assert a.variable_names(store) == b.variable_names(store) == [n for n in names if n.startswith("vgg_16/")]
    assert c.variable_names(store) == [n for n in names if n.startswith("vgg_19/")]
    assert store.specs["vgg_16/fc6/weights"].shape == (7, 7, 32, 64)
    store.finalize()
    w = store["vgg_16/conv2/conv2_1/weights"].numpy()
    lim = np.sqrt(6.0 / (9 * (4 + 8)))                                   # Glorot uniform, fans k k Cin and k k Cout
    assert 0.9 * lim < np.abs(w).max() <= lim and not store["vgg_16/conv2/conv2_1/biases"].numpy().any()
    # initializers= overrides name the variable inside slim's scope
    reset_registry()
    d = make("fourth", spatial_layer="vgg_16/conv1/conv1_1",
             initializers=[("conv1/conv1_1/biases", lambda shape: np.full(shape, 0.5, np.float32))])
    store = VariableStore("cpu", seed=3)
    d.declare_variables(store)
    store.finalize()
    assert (store["vgg_16/conv1/conv1_1/biases"].numpy() == 0.5).all()


# ---- tests/captioning.ini ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def captioning_root(tmp_path_factory):
    return M.extract(tmp_path_factory.mktemp("captioning"))


def test_archives_hold_the_references_bytes(captioning_root):
    names = []
    for bundle in M.IMAGE_BUNDLES:
        assert os.path.getsize(bundle) < 1024 * 1024
        with tarfile.open(bundle) as tar:
            names += [m.name for m in tar.getmembers()]
    jpegs = sorted(n for n in names if n.endswith(".jpg"))
    assert len(jpegs) == 13 and sorted(names) == sorted(jpegs + ["tests/captioning.ini"])
    listed = []
    for split in ("train", "val"):
        with open(os.path.join(captioning_root, "tests", "data", "flickr30k", split + "_images.txt")) as handle:
            listed += ["tests/data/flickr30k/" + line.strip() for line in handle if line.strip()]
    assert sorted(listed) == jpegs
    if os.path.isdir(REF):
        for rel in names:
            with open(os.path.join(REF, rel), "rb") as a, open(os.path.join(captioning_root, rel), "rb") as b:
                assert a.read() == b.read(), rel


def test_captioning_ini_verbatim_reaches_the_references_own_refusal(captioning_root):
    """Without the feature the file fails earlier, with SymbolNotShipped for encoders.imagenet_encoder.ImageNet.  With
    it the [imagenet] section builds, and the decoder over it is refused with the words of the reference
    (decoders/decoder.py:337-342), which cannot build this file either."""
    from neuralmonkey_amd.config.exceptions import ConfigBuildException
    with open(os.path.join(captioning_root, "tests", "captioning.ini")) as handle:
        assert "class=encoders.imagenet_encoder.ImageNet" in handle.read()
    with pytest.raises(ConfigBuildException) as info:
        load_verbatim(captioning_root, "captioning", device="cpu")
    assert M.REFUSAL in str(info.value) and "SymbolNotShipped" not in str(info.value)
    if os.path.isdir(REF):
        text = re.sub(r"[\"']\s*\n\s*[\"']", "", open(os.path.join(REF, "neuralmonkey/decoders/decoder.py")).read())
        assert "The dimension ({}) of the output projection must be same as the dimension of the input embedding ({})" in text


def test_captioning_ini_builds_and_holds_the_frozen_network_to_conv5_3(captioning_root):
    """Fails on a tree without the feature with SymbolNotShipped.  The file with ``rnn_size=9``; on a machine without a
    GPU the images come from the NumPy reader (tests/test_imagenet_gpu.py reads the JPEGs)."""
    from neuralmonkey_amd.attention import Attention
    from neuralmonkey_amd.decoders import Decoder
    from neuralmonkey_amd.encoders import imagenet_encoder as E
    from neuralmonkey_amd.runners import GreedyRunner
    name = M.with_numpy_images(captioning_root, M.with_rnn_size(captioning_root), "captioning_rnn9_numpy")
    model = load_verbatim(captioning_root, name, device="cpu")
    runner, = model.runners
    dec = runner.decoder
    assert isinstance(runner, GreedyRunner) and isinstance(dec, Decoder)
    enc, = dec.encoders
    att, = dec.attentions
    assert type(enc) is E.ImageNet and isinstance(att, Attention) and att.encoder is enc
    assert (enc.name, enc.data_id, enc.network_type, enc.spatial_layer, enc.encoded_layer) == (
        "imagenet_vgg", "images", "vgg_16", "vgg_16/conv5/conv5_3", None)
    assert (enc.dimension, enc.output_size, enc.height, enc.width) == (512, 512, 224, 224)
    assert enc.input_shapes == {"images": [None, 224, 224, 3]} and enc.input_types == {"images": np.float32}
    store = model.tf_manager.sessions[0].store
    upto = []
    for layer in E.layer_table("vgg_16"):
        upto += layer.variables
        if layer.endpoint == "vgg_16/conv5/conv5_3":
            break
    mine = {n: tuple(store[n].shape) for n in store.names() if n.startswith("vgg_16/")}
    assert mine == dict(upto) and len(mine) == 26
    assert sum(int(np.prod(s)) for s in mine.values()) == CONV5_3["vgg_16"]
    assert not any(n.startswith("imagenet_vgg") for n in store.names())
    trainer, = model.trainers
    assert not set(mine) & set(store.trainable_names())
    assert not set(mine) & set(trainer.var_list(store)) and not set(mine) & set(trainer.regularizable(store))
    assert trainer.var_list(store) and trainer.regularizable(store)
    assert enc in trainer.feedables and enc in trainer.parameterizeds
    batch = next(iter(model.train_dataset.batches()))
    assert len(model.train_dataset) == 10 and len(model.val_dataset) == 3 and len(batch) == 5
    fed = enc.feed_dict(batch, train=True)[enc.image_input]
    assert fed.dtype == np.float32 and fed.shape == (5, 224, 224, 3)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_use_the_references_words():
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    from neuralmonkey_amd.runtime import reset_registry
    reset_registry()
    with pytest.raises(ValueError) as info:
        make("a", network_type="vgg_11", spatial_layer="vgg_11/conv5/conv5_3")
    assert str(info.value) == ("Network 'vgg_11' is not among the supported ones (alexnet_v2, vgg_16, vgg_19, "
                               "resnet_v2_50, resnet_v2_101, resnet_v2_152)")
    for i, net in enumerate(("alexnet_v2", "resnet_v2_50", "resnet_v2_101", "resnet_v2_152")):
        with pytest.raises(NotImplementedError) as info:
            make("b{}".format(i), network_type=net, spatial_layer=net + "/whatever")
        assert "'{}'".format(net) in str(info.value) and "strided convolutions" in str(info.value)
        assert "batch normalisation over residual units" in str(info.value)
    cases = [
        (dict(spatial_layer="vgg_16/conv5/conv5_4"), "Network 'vgg_16' does not contain endpoint 'vgg_16/conv5/conv5_4'"),
        (dict(network_type="vgg_19", spatial_layer="vgg_16/conv5/conv5_3"),
         "Network 'vgg_19' does not contain endpoint 'vgg_16/conv5/conv5_3'"),
        (dict(spatial_layer="vgg_16/fc8"), "Endpoint 'vgg_16/fc8' for network 'vgg_16' cannot be a convolutional  map, "
                                           "its dimensionality is: None, 1000."),
        (dict(spatial_layer="vgg_16/pool5", encoded_layer="vgg_16/fc9"),
         "Network 'vgg_16' does not contain endpoint 'vgg_16/fc9'."),
    ]
    for i, (kw, text) in enumerate(cases):
        with pytest.raises(ValueError) as info:
            make("c{}".format(i), **kw)
        assert str(info.value) == text
    own = [
        (dict(), "one of spatial_layer and encoded_layer must be given"),
        (dict(encoded_layer="vgg_16/pool5"), "encoded_layer 'vgg_16/pool5' is a 7 x 7 map"),
        (dict(spatial_layer="vgg_16/pool5", encoded_layer="vgg_16/conv5/conv5_3"), "is a 14 x 14 map"),
        (dict(encoded_layer="vgg_16/fc8"), "encoded_layer 'vgg_16/fc8' is 2-dimensional"),
    ]
    for i, (kw, text) in enumerate(own):
        with pytest.raises(ValueError) as info:
            make("d{}".format(i), **kw)
        assert text in str(info.value), str(info.value)
    with pytest.raises(TypeError):
        make("e", spatial_layer=5)
    with pytest.raises(TypeError):
        make("f", spatial_layer="vgg_16/pool5", slim_models_path=None)
    # encoded_layer alone: no map, no mask
    part = make("g", encoded_layer="vgg_16/fc7")
    assert part.spatial_layer is None and part.output_size == 4096
    with pytest.raises(ValueError):
        part.dimension  # pylint: disable=pointless-statement
    # feed_dict asserts the image size, as the reference does
    part = make("h", spatial_layer="vgg_16/pool5")
    wrong = Dataset("wrong", {"images": [np.zeros((224, 200, 3), np.float32)] * 2}, BatchingScheme(batch_size=2))
    with pytest.raises(AssertionError):
        part.feed_dict(wrong, train=False)
    right = Dataset("right", {"images": [np.zeros((224, 224, 3), np.float32)] * 2}, BatchingScheme(batch_size=2))
    assert part.feed_dict(right, train=False)[part.image_input].shape == (2, 224, 224, 3)
    if os.path.isdir(REF):                                      # the messages are the reference's own text
        text = re.sub(r"[\"']\s*\n\s*[\"']", "", open(os.path.join(REF, "neuralmonkey", PATH)).read())
        for message in ("Network '{}' is not among the supported ones ({})", "Network '{}' does not contain endpoint '{}'",
                        "Network '{}' does not contain endpoint '{}'.",
                        "Endpoint '{}' for network '{}' cannot be a convolutional  map, its dimensionality is: {}."):
            assert message in text, message


def test_slim_models_path_is_never_imported(tmp_path, monkeypatch):
    import sys
    from neuralmonkey_amd.runtime import reset_registry
    reset_registry()
    nets = tmp_path / "nets"
    nets.mkdir()
    (nets / "__init__.py").write_text("raise RuntimeError('imported')\n")
    (nets / "vgg.py").write_text("raise RuntimeError('imported')\n")
    before = list(sys.path)
    make("p", spatial_layer="vgg_16/pool5", slim_models_path=str(tmp_path))
    assert sys.path == before and "nets" not in sys.modules and "nets.vgg" not in sys.modules


# ---- the binding table ------------------------------------------------------------------------------------------------------
def vgg_header_symbols():
    text = open(os.path.join(ROOT, "include", "nmhip_vgg.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nm_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


def test_vgg_header_matches_its_binding_table(lib):
    from neuralmonkey_amd import _lib
    from .test_abi import header_symbols
    from .test_cnn2d_host import image_header_symbols
    mine = vgg_header_symbols()
    assert mine == set(_lib.VGG_SIGNATURES) == {"nm_conv2d_act_fwd"}
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("SIGNATURES") and n != "VGG_SIGNATURES"]
    assert len(others) >= 15 and not any(mine & set(other) for other in others)
    assert not mine & header_symbols() and not mine & image_header_symbols()
    for name, (res, args) in _lib.VGG_SIGNATURES.items():
        fn = getattr(lib, name)                                          # exported, and bound by load()
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    header = open(os.path.join(ROOT, "include", "nmhip_vgg.h")).read()
    prototype = re.search(r"int nm_conv2d_act_fwd\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S)
    kinds = []
    for arg in prototype.group(1).split(","):
        kinds.append(ctypes.c_void_p if "*" in arg else ctypes.c_int64 if "int64_t" in arg else ctypes.c_int)
    assert kinds == list(_lib.VGG_SIGNATURES["nm_conv2d_act_fwd"][1])
    for cited in ("imagenet_encoder.py:212", ":234", "nets/vgg.py"):
        assert cited in header, cited


def test_conv2d_act_refuses_before_any_launch(lib):
    """Host buffers and a null stream: a call that got as far as a launch would fault or fail differently."""
    buf = (ctypes.c_float * 65536)()
    other = (ctypes.c_float * 65536)()
    third = (ctypes.c_float * 65536)()

    def fwd(x=buf, ldx=8, b=2, h=5, w=6, cin=8, filt=third, k=3, cout=4, pad=0, bias=third, relu=1, y=other, ldy=4, algo=0):
        return lib.nm_conv2d_act_fwd(None, x, ldx, b, h, w, cin, filt, k, cout, pad, bias, relu, y, ldy, algo)
    cases = (
        (dict(b=0), b"nm_conv2d_act_fwd: bad sizes B 0, H 5, W 6, Cin 8, Cout 4, k 3"),
        (dict(h=0), b"nm_conv2d_act_fwd: bad sizes B 2, H 0, W 6, Cin 8, Cout 4, k 3"),
        (dict(w=-1), b"nm_conv2d_act_fwd: bad sizes B 2, H 5, W -1, Cin 8, Cout 4, k 3"),
        (dict(cin=0), b"nm_conv2d_act_fwd: bad sizes B 2, H 5, W 6, Cin 0, Cout 4, k 3"),
        (dict(cout=0), b"nm_conv2d_act_fwd: bad sizes B 2, H 5, W 6, Cin 8, Cout 0, k 3"),
        (dict(k=0), b"nm_conv2d_act_fwd: bad sizes B 2, H 5, W 6, Cin 8, Cout 4, k 0"),
        (dict(k=8, h=9, w=9), b"nm_conv2d_act_fwd: the kernel takes k <= 7, not 8"),
        (dict(k=9, pad=1), b"nm_conv2d_act_fwd: the kernel takes k <= 7, not 9"),
        (dict(pad=2), b"nm_conv2d_act_fwd: padding 2 (0 VALID, 1 SAME)"),
        (dict(pad=-1), b"nm_conv2d_act_fwd: padding -1 (0 VALID, 1 SAME)"),
        (dict(h=2), b"nm_conv2d_act_fwd: VALID padding with a 2 x 6 map below the 3 x 3 filter"),
        (dict(w=2), b"nm_conv2d_act_fwd: VALID padding with a 5 x 2 map below the 3 x 3 filter"),
        (dict(b=1 << 20, h=1 << 8, w=1 << 8), b"nm_conv2d_act_fwd: a map or the filter holds more than 2^31 - 1 elements"),
        (dict(x=None), b"nm_conv2d_act_fwd: null pointer"), (dict(filt=None), b"nm_conv2d_act_fwd: null pointer"),
        (dict(y=None), b"nm_conv2d_act_fwd: null pointer"),
        (dict(ldx=7), b"nm_conv2d_act_fwd: ldx 7 below Cin 8"), (dict(ldy=3), b"nm_conv2d_act_fwd: ldy 3 below Cout 4"),
        (dict(y=buf), b"nm_conv2d_act_fwd: y overlapping x"),
        (dict(y=ctypes.byref(buf, 4 * 100)), b"nm_conv2d_act_fwd: y overlapping x"),
        (dict(algo=3), b"nm_conv2d_act_fwd: algo 3 (0 auto, 1 128x64, 2 64x64)"),
        (dict(algo=-1), b"nm_conv2d_act_fwd: algo -1 (0 auto, 1 128x64, 2 64x64)"))
    for kwargs, text in cases:
        assert fwd(**kwargs) < 0 and lib.nm_last_error() == text, (kwargs, lib.nm_last_error())
    # (a null bias is not among the refusals: tests/test_imagenet_kernels_gpu.py runs the kernel without one)


def test_kernels_of_the_vgg_stack_do_not_spill(lib):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_resources
    finally:
        sys.path.pop(0)
    mine = {k: v for k, v in kernel_resources().items() if "vgg_conv_act_mfma" in k}
    assert len(mine) == 4, sorted(mine)                                  # two tiles x vector / scalar gather
    assert all(v["scratch"] == 0 and v["max_threads"] == 256 for v in mine.values())
    assert max(v["lds"] for v in mine.values()) <= 20 * 1024 and max(v["arch_vgprs"] + v["agpr"] for v in mine.values()) <= 256
