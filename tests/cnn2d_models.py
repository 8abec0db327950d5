"""The image encoder of the tests: test infrastructure.

``build``: the engine model of a fixture of tests/golden/cnn2d (make_cnn2d_golden.py) -- a CNNEncoder alone, under a
Classifier, or behind a CNNTemporalView read by a RecurrentEncoder whose SequenceMaxPooling and the view itself feed a
Classifier.  ``np_*`` and ``restate``: a float64 NumPy restatement of the encoder's forward pass, written from
neuralmonkey/encoders/cnn_encoder.py and TensorFlow's documentation; test_cnn2d_host.py holds it against every recorded
tensor, and the kernel tests then use its pieces next to torch's float64 functions."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIX = os.path.join(GOLDEN, "cnn2d")
BUNDLE = os.path.join(GOLDEN, "str_tests.tar.gz")
LISTS = os.path.join(GOLDEN, "cnn2d_signatures.json")
PLAIN_CASES = ["cnn_plain", "cnn_fc"]                                    # one pass, recorded under out/
MODE_CASES = ["cnn_str_stack", "cnn_resnet_same_channels", "cnn_temporal_view"]     # out/infer/ and out/train/
FD_CASES = ["fd_gradients_cnn", "fd_gradients_cnn_temporal"]             # one training-mode pass under out/, and fd/
ALL_CASES = PLAIN_CASES + MODE_CASES + FD_CASES
BOOKKEEPING = ("out/variable_names", "out/variable_shapes", "out/non_trainable")
EPSILON, MOMENTUM = 1e-3, 0.99


def load_fixture(case):
    z = np.load(os.path.join(FIX, case + ".npz"))
    return z, json.loads(str(z["cfg"])), {k[2:]: z[k] for k in z.files if k.startswith("p/")}


def passes(case, cfg):
    """[(prefix of the recorded tensors, train_mode)] of a fixture."""
    if case in MODE_CASES:
        return [("out/infer/", False), ("out/train/", True)]
    return [("out/", bool(cfg["train_mode"]))]


def recorded(z, prefix):
    """name -> array of the tensors recorded under ``prefix`` (the other pass and the bookkeeping aside)."""
    out = {}
    for key in z.files:
        if not key.startswith(prefix) or key in BOOKKEEPING:
            continue
        rest = key[len(prefix):]
        if prefix == "out/" and rest.split("/")[0] in ("infer", "train"):
            continue
        out[rest] = z[key]
    return out


# ---- the engine's model ---------------------------------------------------------------------------------------------------
def words(n):
    from neuralmonkey_amd.vocabulary import Vocabulary
    return Vocabulary(["w{}".format(i) for i in range(n)])


def build_parts(cfg):
    """The model parts of a fixture's configuration; no session."""
    from neuralmonkey_amd import tf_shim
    from neuralmonkey_amd.decoders import Classifier
    from neuralmonkey_amd.encoders import RecurrentEncoder, SequenceMaxPooling
    from neuralmonkey_amd.encoders.cnn_encoder import CNNEncoder, CNNTemporalView
    from neuralmonkey_amd.runtime import reset_registry
    reset_registry()
    cnn = CNNEncoder(name="cnn", data_id="images", convolutions=[tuple(s) for s in cfg["convolutions"]],
                     image_height=cfg["height"], image_width=cfg["width"], pixel_dim=cfg["pixel_dim"],
                     fully_connected=cfg["fully_connected"], batch_normalize=cfg["batch_normalize"], dropout_keep_prob=1.0)
    m = dict(cnn=cnn, view=None, enc=None, pool=None, dec=None, feedables=[cnn])
    readers = [cnn]
    if cfg["head"] == "temporal":
        m["view"] = CNNTemporalView(name="cnn_in_time", cnn=cnn)
        m["enc"] = RecurrentEncoder(name="encoder", input_sequence=m["view"],
                                    rnn_layers=[(cfg["rnn_size"], "forward", "GRU")])
        m["pool"] = SequenceMaxPooling(name="encoder_max", input_sequence=m["enc"])
        m["feedables"] += [m["view"], m["enc"], m["pool"]]
        readers = [m["pool"], m["view"]]
    if cfg["head"] is not None:
        m["dec"] = Classifier(name="classifier", encoders=readers, vocabulary=words(cfg["cls_vocab"]), data_id="target",
                              layers=cfg["layers"], activation_fn=tf_shim.tanh, dropout_keep_prob=1.0)
        m["feedables"].append(m["dec"])
    return m


def build(dev, cfg):
    from neuralmonkey_amd.tf_manager import TensorFlowManager
    from neuralmonkey_amd.trainers import CrossEntropyTrainer
    m = build_parts(cfg)
    m["trainer"] = None
    if m["dec"] is not None:
        m["trainer"] = CrossEntropyTrainer(decoders=[m["dec"]], l2_weight=0.0, clip_norm=None)
    tfm = TensorFlowManager(num_sessions=1, num_threads=1, device=str(dev), seed=1)
    tfm.initialize_sessions()
    m.update(tfm=tfm, store=tfm.sessions[0].store)
    return m


def dataset_of(z, cfg):
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    images = [np.asarray(im) for im in z["in/images"]]
    series = {"images": images}
    if cfg["head"] is not None:
        series["target"] = [[str(t)] for t in z["in/tgt_tokens"]]
    return Dataset("fixture", series, BatchingScheme(batch_size=len(images)))


def loaded(dev, case):
    from .test_reference_exec_gpu import load_variables
    z, cfg, params = load_fixture(case)
    m = build(dev, cfg)
    assert load_variables(m["store"], params) == []              # the same variables under the same names, both ways
    ds = dataset_of(z, cfg)
    return z, cfg, params, m, ds


def feed(m, ds, train):
    fd = {}
    for part in m["feedables"]:
        fd.update(part.feed_dict(ds, train=train))
    return fd


# ---- float64 NumPy restatement ----------------------------------------------------------------------------------------------
def np_pad(size, k, stride, padding):
    """(output size, padded positions before the map) of one axis: TensorFlow's SAME / VALID arithmetic."""
    if padding == "valid":
        return (size - k) // stride + 1, 0
    out = -(-size // stride)
    return out, max((out - 1) * stride + k - size, 0) // 2


def np_conv2d(x, w, bias, padding):
    """tf.layers.conv2d at stride 1: x [B, H, W, Cin], w [k, k, Cin, Cout]."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    bsz, h, wid, cin = x.shape
    k, cout = w.shape[0], w.shape[3]
    oh, pt = np_pad(h, k, 1, padding)
    ow, pl = np_pad(wid, k, 1, padding)
    out = np.zeros((bsz, oh, ow, cout)) + (0.0 if bias is None else np.asarray(bias, np.float64))
    for oy in range(oh):
        for ox in range(ow):
            for ky in range(k):
                for kx in range(k):
                    iy, ix = oy + ky - pt, ox + kx - pl
                    if 0 <= iy < h and 0 <= ix < wid:
                        out[:, oy, ox] += x[:, iy, ix] @ w[ky, kx]
    return out


def np_window2d(x, window, stride, padding, mode):
    """max / average pooling; -> (pooled, flat index iy * W + ix of each window's FIRST maximum in row-major order)."""
    x = np.asarray(x, np.float64)
    bsz, h, wid, c = x.shape
    oh, pt = np_pad(h, window[0], stride[0], padding)
    ow, pl = np_pad(wid, window[1], stride[1], padding)
    out = np.zeros((bsz, oh, ow, c))
    where = np.zeros((bsz, oh, ow, c), np.int64)
    for oy in range(oh):
        for ox in range(ow):
            ys = [y for y in range(oy * stride[0] - pt, oy * stride[0] - pt + window[0]) if 0 <= y < h]
            xs = [v for v in range(ox * stride[1] - pl, ox * stride[1] - pl + window[1]) if 0 <= v < wid]
            flat = np.asarray([y * wid + v for y in ys for v in xs])
            win = x[:, ys][:, :, xs].reshape(bsz, len(flat), c)
            if mode == "max":
                first = win.argmax(axis=1)                       # NumPy's argmax takes the first of equals
                out[:, oy, ox] = np.take_along_axis(win, first[:, None, :], axis=1)[:, 0]
                where[:, oy, ox] = flat[first]
            else:
                out[:, oy, ox] = win.mean(axis=1)
    return out, where


def np_batch_norm(x, gamma, beta, mean, var):
    return (np.asarray(x, np.float64) - mean) / np.sqrt(var + EPSILON) * gamma + beta


def restate(cfg, params, images, train):
    """The CNN's forward pass -> dict of what the fixtures record for it (``stats/...`` in training mode)."""
    p = {k: np.asarray(v, np.float64) for k, v in params.items()}
    out = {}
    x = np.asarray(images, np.float64) / 255.0
    mask = np.sign(x.sum(axis=3, keepdims=True))
    out["image_mask"] = mask

    def bn(t, scope):
        if not cfg["batch_normalize"]:
            return t
        pre = "cnn/" + scope + "/batch_normalization/"
        if train:
            mean, var = t.mean(axis=(0, 1, 2)), t.var(axis=(0, 1, 2))
            out["stats/" + pre + "batch_mean"], out["stats/" + pre + "batch_variance"] = mean, var
        else:
            mean, var = p[pre + "moving_mean"], p[pre + "moving_variance"]
        return np_batch_norm(t, p[pre + "gamma"], p[pre + "beta"], mean, var)

    def conv(t, scope, padding):
        return np_conv2d(t, p["cnn/" + scope + "/conv2d/kernel"], p["cnn/" + scope + "/conv2d/bias"], padding)

    channels = cfg["pixel_dim"]
    for i, spec in enumerate(cfg["convolutions"]):
        if spec[0] == "C":
            _, k, stride, pad, channels = spec
            scope = "convolutions/layer_{}_convolution".format(i)
            x = np.maximum(bn(conv(x, scope, pad), scope), 0.0)
            mask = np_window2d(mask, (k, k), (stride, stride), pad, "max")[0]
        elif spec[0] in ("M", "A"):
            _, size, stride, _ = spec
            x = np_window2d(x, (size, size), (stride, stride), "valid", "max" if spec[0] == "M" else "avg")[0]
            mask = np_window2d(mask, (size, size), (stride, stride), "valid", "max")[0]
        else:
            _, k, out_channels = spec
            scope = "convolutions/layer_{}_resnet_block".format(i)
            before = x
            if out_channels != channels:
                before = bn(conv(x, scope + "/project_input", "same"), scope + "/project_input")
            after = conv(np.maximum(bn(x, scope + "/conv_a"), 0.0), scope + "/conv_a", "same")
            after = conv(np.maximum(bn(after, scope + "/conv_b"), 0.0), scope + "/conv_b", "same")
            x, channels = after + before, out_channels
        out["layer_{}_states".format(i)], out["layer_{}_mask".format(i)] = x, mask
    out["spatial_states"], out["spatial_mask"] = x, mask
    if cfg["fully_connected"] is None:
        out["output"] = x.mean(axis=(1, 2))
    else:
        y = x.reshape(x.shape[0], -1)
        for i, _ in enumerate(cfg["fully_connected"]):
            y = np.maximum(y @ p["cnn/mlp/mlp_layer_{}/kernel".format(i)] + p["cnn/mlp/mlp_layer_{}/bias".format(i)], 0.0)
        out["output"] = y
    bsz, h, w, c = x.shape
    out["temporal_states"] = x.transpose(0, 2, 1, 3).reshape(bsz, w, h * c)
    out["temporal_mask"] = (mask[..., 0].sum(axis=1) > 0).astype(np.float64)
    return out
