"""Generate ``tests/golden/cnn2d/*.npz``: the image encoder run by the REFERENCE'S OWN Python.

Runs only where the reference tree is (nothing at test time needs it).  It imports the helpers of
``make_reference_exec_golden.py`` -- the NumPy-eager TensorFlow stand-in, the name-seeded variable factory, ``save`` --
and ``neuralmonkey.encoders.cnn_encoder`` UNMODIFIED (plus ``encoders.recurrent``, ``encoders.pooling`` and
``decoders.classifier`` for the cases that read the encoder).  The fixtures have the layout of ``tests/golden/ref_exec``
(``cfg``, ``p/<variable>``, ``in/*``, ``out/*``) in a directory of their own.

The stand-in knows only the 1x1 ``conv2d``; this file supplies NumPy restatements of what cnn_encoder.py calls:
``tf.layers.conv2d`` (any square kernel, stride 1, SAME / VALID: of the k - 1 padded rows (k - 1) // 2 lie before the map),
``tf.layers.batch_normalization`` (TensorFlow's defaults: momentum 0.99, epsilon 1e-3, centre and scale, last axis;
training: the batch's mean and BIASED variance; inference: the moving statistics) and ``tf.layers.max_pooling2d`` /
``average_pooling2d`` (padded positions take no part).  They are ``tf_eager.Layer`` subclasses, so variables get the names
TensorFlow gives them.

The stand-in computes in float32.  Everything here runs in FLOAT64 instead: ``tf.float32`` is mapped to NumPy's float64
for the time of the generation and the stand-in's conversions are kept from narrowing, so that the recorded outputs can
be restated to 1e-9 and central differences can take a step of 1e-6.

    python tests/golden/make_cnn2d_golden.py            # all cases
    python tests/golden/make_cnn2d_golden.py cnn_plain

Every batch: 3 images (12 x 20 x 1, 8 x 20 x 1 or 10 x 14 x 3) with pixel values in [0, 255]; image 1 is all zero in its right third, so masks are not all ones.
"""
import collections
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_exec_golden as G  # noqa: E402  pylint: disable=wrong-import-position

assert os.path.isdir(os.path.join(G.REFERENCE, "neuralmonkey")), "the reference tree is not here"

tf, tf_eager = G.tf, G.tf_eager
OUT = os.path.join(HERE, "cnn2d")
G.OUT = OUT

# ---- float64 throughout ---------------------------------------------------------------------------------------------------
tf_eager.float32._np = np.float64                    # pylint: disable=protected-access
_convert32 = tf_eager._convert                       # pylint: disable=protected-access
_get_variable32 = tf_eager.get_variable


def _convert64(x, dtype=None):
    v = _convert32(x, dtype)
    return v.astype(np.float64) if v.dtype == np.float32 else v


def _get_variable64(name, shape=None, dtype=None, **kwargs):
    return _get_variable32(name, shape=shape, dtype=tf.float32 if dtype is None else dtype, **kwargs)


tf_eager._convert = _convert64                       # pylint: disable=protected-access
tf_eager.get_variable = tf.get_variable = _get_variable64

EPSILON, MOMENTUM = 1e-3, 0.99
BATCH_STATS = collections.OrderedDict()              # "<scope>/batch_{mean,variance}" of the last training-mode pass
PRE_RELU = []                                        # what a ReLU of cnn_encoder.py saw
POOL_GAPS = []                                       # per max window: the best value minus the runner-up


def _np(x):
    return np.asarray(x.numpy() if hasattr(x, "numpy") else x, np.float64)


def pad_amounts(size, k, stride, padding):
    """(output size, padded before) of one axis, TensorFlow's arithmetic."""
    if padding == "valid":
        return (size - k) // stride + 1, 0
    out = -(-size // stride)
    return out, max((out - 1) * stride + k - size, 0) // 2


def conv2d_np(x, w, padding):
    """x [B, H, W, Cin], w [k, k, Cin, Cout], stride 1."""
    k = w.shape[0]
    bsz, h, wid, _ = x.shape
    oh, pt = pad_amounts(h, k, 1, padding)
    ow, pl = pad_amounts(wid, k, 1, padding)
    padded = np.zeros((bsz, h + k - 1, wid + k - 1, x.shape[3]))
    padded[:, pt:pt + h, pl:pl + wid] = x
    out = np.zeros((bsz, oh, ow, w.shape[3]))
    for ky in range(k):
        for kx in range(k):
            out += padded[:, ky:ky + oh, kx:kx + ow] @ w[ky, kx]
    return out


def pool_np(x, size, stride, padding, mode, gaps=None):
    bsz, h, wid, c = x.shape
    oh, pt = pad_amounts(h, size, stride, padding)
    ow, pl = pad_amounts(wid, size, stride, padding)
    out = np.zeros((bsz, oh, ow, c))
    for oy in range(oh):
        for ox in range(ow):
            y0, x0 = max(oy * stride - pt, 0), max(ox * stride - pl, 0)
            y1, x1 = min(oy * stride - pt + size, h), min(ox * stride - pl + size, wid)
            win = x[:, y0:y1, x0:x1].reshape(bsz, -1, c)
            out[:, oy, ox] = win.max(axis=1) if mode == "max" else win.mean(axis=1)
            if gaps is not None and mode == "max" and win.shape[1] > 1:
                # Not counted: windows whose maximum is a ReLU's zero (they carry no gradient), and candidates that are
                # EXACTLY equal -- the blank third of image 1 gives every position there the same value, whatever the
                # variables are, so such a tie stays a tie under every perturbation and the cost has no kink at it.
                top = np.sort(win, axis=1)
                gap = np.where((top[:, -1] > 0.0) & (top[:, -1] != top[:, -2]), top[:, -1] - top[:, -2], np.inf)
                gaps.append(float(gap.min()))
    return out


class Conv2D(tf_eager.Layer):
    """tf.layers.Conv2D at stride 1."""

    def __init__(self, filters, kernel_size, padding="valid", name=None, **kwargs):
        super().__init__(name=name, **kwargs)
        self.filters, self.k, self.padding = int(filters), int(kernel_size), padding

    def build(self, input_shape):
        depth = tf_eager.TensorShape(input_shape)[-1].value
        self.kernel = self.add_variable("kernel", [self.k, self.k, depth, self.filters])
        self.bias = self.add_variable("bias", [self.filters], initializer=tf_eager.zeros_initializer())
        self.built = True

    def call(self, inputs):
        return tf_eager.Tensor(conv2d_np(_np(inputs), _np(self.kernel), self.padding) + _np(self.bias))


class BatchNormalization(tf_eager.Layer):
    def build(self, input_shape):
        depth = tf_eager.TensorShape(input_shape)[-1].value
        self.gamma = self.add_variable("gamma", [depth], initializer=tf_eager.ones_initializer())
        self.beta = self.add_variable("beta", [depth], initializer=tf_eager.zeros_initializer())
        self.moving_mean = self.add_variable("moving_mean", [depth], initializer=tf_eager.zeros_initializer(),
                                             trainable=False)
        self.moving_variance = self.add_variable("moving_variance", [depth], initializer=tf_eager.ones_initializer(),
                                                 trainable=False)
        self.built = True

    def call(self, inputs, training=False):
        x = _np(inputs)
        if bool(np.asarray(training.numpy() if hasattr(training, "numpy") else training)):
            mean, var = x.mean(axis=(0, 1, 2)), x.var(axis=(0, 1, 2))
            BATCH_STATS[self.scope_name + "/batch_mean"] = mean
            BATCH_STATS[self.scope_name + "/batch_variance"] = var
        else:
            mean, var = _np(self.moving_mean), _np(self.moving_variance)
        return tf_eager.Tensor((x - mean) / np.sqrt(var + EPSILON) * _np(self.gamma) + _np(self.beta))


def layers_conv2d(inputs, filters, kernel_size, strides=(1, 1), padding="valid", activation=None, name=None, **_):
    assert strides in (1, (1, 1)) and activation is None, (strides, activation)
    return Conv2D(filters, kernel_size, padding=padding, name=name, _scope=name).apply(inputs)


def layers_batch_normalization(inputs, training=False, name=None, **_):
    return BatchNormalization(name=name, _scope=name).apply(inputs, training=training)


def layers_max_pooling2d(inputs, pool_size, strides, padding="valid", **_):
    x = _np(inputs)
    return tf_eager.Tensor(pool_np(x, int(pool_size), int(strides), padding, "max",
                                   gaps=POOL_GAPS if x.shape[3] > 1 or not set(np.unique(x)) <= {0.0, 1.0} else None))


def layers_average_pooling2d(inputs, pool_size, strides, padding="valid", **_):
    return tf_eager.Tensor(pool_np(_np(inputs), int(pool_size), int(strides), padding, "avg"))


_relu = tf.nn.relu


def watched_relu(x, *args, **kwargs):
    PRE_RELU.append(_np(x).copy())
    return _relu(x, *args, **kwargs)


def assert_greater(x, y, *_args, **_kwargs):
    """tf.assert_greater (encoders/pooling.py:49) for the eager stand-in: checked at once."""
    if not np.all(_np(x) > _np(y)):
        raise ValueError("assert_greater failed: {} > {}".format(_np(x), _np(y)))


tf.assert_greater = assert_greater
tf.layers.conv2d = layers_conv2d
tf.layers.batch_normalization = layers_batch_normalization
tf.layers.max_pooling2d = layers_max_pooling2d
tf.layers.average_pooling2d = layers_average_pooling2d


def variable_factory(name, shape, np_dtype, initializer):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name.endswith("moving_variance"):
        return rng.uniform(0.5, 1.5, shape).astype(np_dtype)
    if name.endswith("moving_mean"):
        return rng.normal(0, 0.3, shape).astype(np_dtype)
    return G.variable_factory(name, shape, np_dtype, initializer)


tf_eager.VARIABLE_FACTORY = variable_factory

STR_STACK = [["C", 3, 1, "valid", 4], ["M", 2, 2, "same"], ["R", 3, 12], ["A", 2, 1, "same"]]
PLAIN_STACK = [["C", 3, 1, "valid", 5], ["M", 2, 2, "valid"], ["C", 2, 1, "same", 6], ["A", 2, 1, "valid"]]
DEFAULT = dict(height=12, width=20, pixel_dim=1, convolutions=PLAIN_STACK, fully_connected=None, batch_normalize=False,
               head=None, train_mode=False, cls_vocab=5, layers=[6], rnn_size=5, seed=61, batch=3)


def specs(cfg):
    return [tuple(s) for s in cfg["convolutions"]]


def build(cfg):
    from neuralmonkey.encoders.cnn_encoder import CNNEncoder, CNNTemporalView
    cnn = CNNEncoder(name="cnn", data_id="images", convolutions=specs(cfg), image_height=cfg["height"],
                     image_width=cfg["width"], pixel_dim=cfg["pixel_dim"], fully_connected=cfg["fully_connected"],
                     batch_normalize=cfg["batch_normalize"], dropout_keep_prob=1.0)
    m = dict(cnn=cnn, view=None, enc=None, pool=None, dec=None, parts=[cnn])
    readers = [cnn]
    if cfg["head"] == "temporal":
        from neuralmonkey.encoders.pooling import SequenceMaxPooling
        from neuralmonkey.encoders.recurrent import RecurrentEncoder
        m["view"] = CNNTemporalView(name="cnn_in_time", cnn=cnn)
        m["enc"] = RecurrentEncoder(name="encoder", input_sequence=m["view"], rnn_layers=[(cfg["rnn_size"], "forward", "GRU")])
        m["pool"] = SequenceMaxPooling(name="encoder_max", input_sequence=m["enc"])
        m["parts"] += [m["view"], m["enc"], m["pool"]]
        readers = [m["pool"], m["view"]]
    if cfg["head"] is not None:
        from neuralmonkey.decoders.classifier import Classifier
        m["dec"] = Classifier(name="classifier", encoders=readers, vocabulary=G.make_vocab(cfg["cls_vocab"]),
                              data_id="target", layers=cfg["layers"], activation_fn=tf.tanh, dropout_keep_prob=1.0)
        m["parts"].append(m["dec"])
    return m


def series_of(cfg):
    rng = np.random.default_rng(cfg["seed"])
    images = rng.uniform(1.0, 255.0, (cfg["batch"], cfg["height"], cfg["width"], cfg["pixel_dim"]))
    images[1, :, cfg["width"] - cfg["width"] // 3:] = 0.0
    tgt = [["w{}".format(int(rng.integers(0, cfg["cls_vocab"])))] for _ in range(cfg["batch"])]
    return {"images": [im for im in images], "target": tgt}


def inputs_of(cfg):
    return {"images": tf.placeholder(tf.float32, [None, cfg["height"], cfg["width"], cfg["pixel_dim"]], "images"),
            "target": tf.placeholder(tf.string, [None], "target")}


def feed(m, cfg, ds):
    return G.feed(m["parts"], ds, cfg["train_mode"], inputs_of(cfg))


def forward(cfg, series, out, tag="out/", per_layer=True):
    G.fresh_graph()
    BATCH_STATS.clear()
    m = build(cfg)
    ds = G.dataset(series)
    cnn = m["cnn"]
    with tf_eager.feeding(feed(m, cfg, ds)):
        out["in/images"] = np.asarray(series["images"])
        out[tag + "image_mask"] = cnn.image_mask.numpy()
        for i, (states, mask) in enumerate(cnn.image_processing_layers if per_layer else []):
            out[tag + "layer_{}_states".format(i)] = states.numpy()
            out[tag + "layer_{}_mask".format(i)] = mask.numpy()
        out[tag + "spatial_states"] = cnn.spatial_states.numpy()
        out[tag + "spatial_mask"] = cnn.spatial_mask.numpy()
        out[tag + "output"] = cnn.output.numpy()
        if m["view"] is not None:
            out[tag + "temporal_states"] = m["view"].temporal_states.numpy()
            out[tag + "temporal_mask"] = m["view"].temporal_mask.numpy()
            out[tag + "enc_states"] = m["enc"].temporal_states.numpy()
            out[tag + "enc_output"] = m["enc"].output.numpy()
            out[tag + "pool_output"] = m["pool"].output.numpy()
        if m["dec"] is not None:
            out["in/tgt_tokens"] = np.asarray(m["dec"].targets.numpy())
            out["in/tgt_ids"] = m["dec"].gt_inputs.numpy()
            out[tag + "decoded_logits"] = m["dec"].decoded_logits.numpy()
            out[tag + "cost"] = m["dec"].cost.numpy()
    for key, val in BATCH_STATS.items():
        out[tag + "stats/" + key] = val
    order, params = G.variables()
    out["out/variable_names"] = np.asarray(order)
    out["out/variable_shapes"] = np.asarray([json.dumps(list(params[n].shape)) for n in order])
    out["out/non_trainable"] = np.asarray([v.name.split(":")[0] for v in tf_eager.global_variables() if not v.trainable])
    return m


def run_forward(case, **overrides):
    cfg = dict(DEFAULT, **overrides)
    out = {}
    forward(cfg, series_of(cfg), out)
    G.save(case, cfg, out)


def run_both_modes(case, per_layer=True, **overrides):
    """One stack in training mode (batch statistics, recorded) and in inference mode (the moving statistics of p/)."""
    cfg = dict(DEFAULT, **overrides)
    out = {}
    forward(dict(cfg, train_mode=False), series_of(cfg), out, tag="out/infer/", per_layer=False)
    forward(dict(cfg, train_mode=True), series_of(cfg), out, tag="out/train/", per_layer=per_layer)
    G.save(case, cfg, out)


def run_fd(case, per_variable=3, h=1e-6, **overrides):
    """Central differences of the reference's ``cost`` (train mode: batch statistics) at ``per_variable`` coordinates of
    every trainable variable.  Generation fails when a pre-activation behind a ReLU, or the two best candidates of a
    max-pooling window, lie closer than 100 steps to a tie: the cost would have a kink between the two evaluations."""
    cfg = dict(DEFAULT, train_mode=True, **overrides)
    series = series_of(cfg)
    ds = G.dataset(series)
    bump = {}

    def factory(name, shape, np_dtype, initializer):
        value = variable_factory(name, shape, np_dtype, initializer)
        if name in bump:
            idx, delta = bump[name]
            value = value.copy()
            value.reshape(-1)[idx] += np.asarray(delta, value.dtype)
        return value

    def loss():
        G.fresh_graph()
        m = build(cfg)
        with tf_eager.feeding(feed(m, cfg, ds)):
            return float(m["dec"].cost.numpy())
    tf_eager.VARIABLE_FACTORY = factory
    tf.nn.relu = watched_relu
    try:
        out = {}
        del PRE_RELU[:], POOL_GAPS[:]
        forward(cfg, series, out)
        margin = 100.0 * h
        nearest = min(float(np.abs(a).min()) for a in PRE_RELU)
        assert nearest > margin, "{}: a ReLU input at {:.3g} from zero; choose another seed".format(case, nearest)
        assert min(POOL_GAPS or [np.inf]) > margin, "{}: two maxima of a window {:.3g} apart; choose another seed".format(
            case, min(POOL_GAPS))
        out["fd/relu_margin"], out["fd/max_margin"] = np.asarray(nearest), np.asarray(min(POOL_GAPS or [np.inf]))
        tf.nn.relu = _relu
        order, params = G.variables()
        frozen = set(out["out/non_trainable"].tolist())
        rng = np.random.default_rng(zlib.crc32(case.encode()))
        names, index, value = [], [], []
        for name in order:
            v = params[name]
            if v.dtype.kind != "f" or v.size == 0 or name in frozen:
                continue
            for i in rng.choice(v.size, size=min(per_variable, v.size), replace=False):
                bump.clear()
                bump[name] = (int(i), +h)
                up = loss()
                bump[name] = (int(i), -h)
                down = loss()
                names.append(name)
                index.append(int(i))
                value.append((up - down) / (2.0 * h))
        bump.clear()
        loss()                                   # leave the unperturbed variables in the store for save()
        out["fd/names"] = np.asarray(names)
        out["fd/index"] = np.asarray(index, np.int64)
        out["fd/value"] = np.asarray(value, np.float64)
        out["fd/h"] = np.asarray(h)
    finally:
        tf_eager.VARIABLE_FACTORY = variable_factory
        tf.nn.relu = _relu
    G.save(case, cfg, out)


def write_signatures():
    """tests/golden/cnn2d_signatures.json: the constructor parameters of the reference's classes."""
    sys.path.insert(0, os.path.join(G.REPO))
    from tests.test_reference_signatures import read_reference_parameters
    path = "encoders/cnn_encoder.py"
    lists = {path: {cls: read_reference_parameters(path, cls) for cls in ("CNNEncoder", "CNNTemporalView")}}
    with open(os.path.join(HERE, "cnn2d_signatures.json"), "w", encoding="utf-8") as handle:
        json.dump(lists, handle, indent=1, sort_keys=True)
        handle.write("\n")


STR_MEMBERS = ("tests/str.ini", "tests/data/str/vocab.tsv", "tests/data/str/train_files.txt",
               "tests/data/str/train_words.txt", "tests/data/str/val_files.txt", "tests/data/str/val_words.txt")


def write_bundle():
    """tests/golden/str_tests.tar.gz: tests/str.ini, its vocabulary and the four lists it names, byte for byte (the
    images themselves are not bundled)."""
    import gzip
    import io
    import tarfile
    raw = io.BytesIO()
    with tarfile.open(fileobj=raw, mode="w", format=tarfile.GNU_FORMAT) as tar:
        for rel in STR_MEMBERS:
            with open(os.path.join(G.REFERENCE, rel), "rb") as handle:
                data = handle.read()
            info = tarfile.TarInfo(rel)
            info.size, info.mode, info.mtime = len(data), 0o644, 0
            tar.addfile(info, io.BytesIO(data))
    with open(os.path.join(HERE, "str_tests.tar.gz"), "wb") as handle:
        with gzip.GzipFile(fileobj=handle, mode="wb", mtime=0, filename="") as gz:
            gz.write(raw.getvalue())


RESNET_SAME = [["C", 3, 1, "valid", 4], ["R", 3, 4], ["A", 2, 1, "same"]]
TEMPORAL = [["C", 3, 1, "valid", 4], ["M", 2, 2, "same"], ["R", 3, 6]]
RGB = dict(height=10, width=14, pixel_dim=3)

CASES = collections.OrderedDict([
    ("cnn_plain", lambda c: run_forward(c)),
    ("cnn_fc", lambda c: run_forward(c, fully_connected=[9, 5], seed=62)),
    ("cnn_str_stack", lambda c: run_both_modes(c, convolutions=STR_STACK, batch_normalize=True, seed=63, height=8)),
    ("cnn_resnet_same_channels", lambda c: run_both_modes(c, convolutions=RESNET_SAME, batch_normalize=True, seed=64,
                                                          **RGB)),
    ("cnn_temporal_view", lambda c: run_both_modes(c, convolutions=TEMPORAL, batch_normalize=True, head="temporal",
                                                   seed=65, per_layer=False, **RGB)),
    ("fd_gradients_cnn", lambda c: run_fd(c, convolutions=RESNET_SAME, batch_normalize=True, head="classifier",
                                          seed=66, **RGB)),
    ("fd_gradients_cnn_temporal", lambda c: run_fd(c, convolutions=TEMPORAL, batch_normalize=True, head="temporal",
                                                   seed=67, **RGB)),
])


if __name__ == "__main__":
    for name_ in (sys.argv[1:] or list(CASES)):
        CASES[name_](name_)
    if not sys.argv[1:]:
        write_signatures()
        write_bundle()
