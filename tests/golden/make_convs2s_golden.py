"""Generate ``tests/golden/convs2s/*.npz``: the convolutional sequence-to-sequence encoder run by the REFERENCE'S OWN
Python.

Runs only where the reference tree is (nothing at test time needs it).  It imports the helpers of
``make_reference_exec_golden.py`` -- the NumPy-eager TensorFlow stand-in, the name-seeded variable factory, ``save`` --
and ``neuralmonkey.encoders.facebook_conv`` UNMODIFIED (plus ``encoders.pooling`` and ``decoders.classifier`` for the
case that reads the encoder).  The fixtures have the layout of ``tests/golden/ref_exec`` (``cfg``, ``p/<variable>``,
``in/*``, ``out/*``) in a directory of their own.

The stand-in has no ``tf.nn.conv1d``; this file supplies one: a NumPy restatement of stride 1, "SAME" -- (w - 1) // 2
zero positions before the sentence, the rest after.

    python tests/golden/make_convs2s_golden.py            # all cases
    python tests/golden/make_convs2s_golden.py convs2s_k5

Every batch: 5 ragged sentences of lengths [4, 7, 3, 6, 1] over 17 source words, one with an unknown word; embeddings
of 6.
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
OUT = os.path.join(HERE, "convs2s")
G.OUT = OUT


def conv1d(value, filters, stride, padding, *_args, **_kwargs):
    """tf.nn.conv1d for the eager stand-in: value [B, T, Cin], filters [w, Cin, Cout], stride 1, "SAME"."""
    assert stride == 1 and padding == "SAME", (stride, padding)
    x = value.numpy() if hasattr(value, "numpy") else np.asarray(value)
    w = filters.numpy() if hasattr(filters, "numpy") else np.asarray(filters)
    width = w.shape[0]
    before = (width - 1) // 2
    steps = x.shape[1]
    padded = np.pad(x, ((0, 0), (before, width - 1 - before), (0, 0)))
    out = np.zeros(x.shape[:2] + (w.shape[2],), np.result_type(x, w))
    for k in range(width):
        out += padded[:, k:k + steps] @ w[k]
    return tf_eager.Tensor(out)


tf.nn.conv1d = conv1d

LENGTHS = [4, 7, 3, 6, 1]

DEFAULT = dict(src_vocab=17, cls_vocab=6, emb=6, conv_features=10, encoder_layers=2, kernel_width=5, max_length=9,
               head=None, layers=[], activation="tanh", seed=41, batch=5)


def build(cfg):
    from neuralmonkey.encoders.facebook_conv import SentenceEncoder
    from neuralmonkey.model.sequence import EmbeddedSequence
    seq = EmbeddedSequence(name="encoder_input", vocabulary=G.make_vocab(cfg["src_vocab"]), data_id="source",
                           embedding_size=cfg["emb"], max_length=cfg["max_length"])
    enc = SentenceEncoder(name="encoder", input_sequence=seq, conv_features=cfg["conv_features"],
                          encoder_layers=cfg["encoder_layers"], kernel_width=cfg["kernel_width"])
    parts, avg, dec = [seq, enc], None, None
    if cfg["head"] == "classifier":
        from neuralmonkey.decoders.classifier import Classifier
        from neuralmonkey.encoders.pooling import SequenceAveragePooling
        avg = SequenceAveragePooling(name="encoder_avg", input_sequence=enc)
        act = {"relu": tf.nn.relu, "tanh": tf.tanh}[cfg["activation"]]
        dec = Classifier(name="classifier", encoders=[enc, avg], vocabulary=G.make_vocab(cfg["cls_vocab"]),
                         data_id="target", layers=cfg["layers"], activation_fn=act, dropout_keep_prob=1.0)
        parts += [avg, dec]
    return seq, enc, avg, dec, parts


def series_of(cfg):
    rng = np.random.default_rng(cfg["seed"])
    src = [["w{}".format(int(rng.integers(0, cfg["src_vocab"]))) for _ in range(n)] for n in LENGTHS]
    src[0][1] = "never-seen"
    tgt = [["w{}".format(int(rng.integers(0, cfg["cls_vocab"])))] for _ in src]
    tgt[0] = ["never-seen"]
    return {"source": src, "target": tgt}


def inputs_of():
    inputs = G.string_inputs("source")
    inputs["target"] = tf.placeholder(tf.string, [None], "target")
    return inputs


def forward(cfg, series, out):
    G.fresh_graph()
    seq, enc, avg, dec, parts = build(cfg)
    ds = G.dataset(series)
    with tf_eager.feeding(G.feed(parts, ds, False, inputs_of())):
        out["in/src_sentences"] = np.asarray([" ".join(s) for s in series["source"]])      # before max_length cuts
        out["in/src_tokens"] = seq.input_factors[0].numpy()
        out["in/src_ids"] = seq.inputs.numpy()
        out["out/ordered_embedded_inputs"] = enc.ordered_embedded_inputs.numpy()
        out["out/temporal_states"] = enc.temporal_states.numpy()
        out["out/temporal_mask"] = enc.temporal_mask.numpy()
        out["out/output"] = enc.output.numpy()
        if dec is not None:
            out["in/tgt_tokens"] = np.asarray(dec.targets.numpy())
            out["in/tgt_ids"] = dec.gt_inputs.numpy()
            out["out/avg_output"] = avg.output.numpy()
            out["out/decoded_seq"] = dec.decoded_seq.numpy()
            out["out/decoded_logits"] = dec.decoded_logits.numpy()
            out["out/cost"] = dec.cost.numpy()
    order, params = G.variables()
    out["out/variable_names"] = np.asarray(order)
    out["out/variable_shapes"] = np.asarray([json.dumps(list(params[n].shape)) for n in order])
    return enc, dec, parts


def run_forward(case, **overrides):
    cfg = dict(DEFAULT, **overrides)
    out = {}
    forward(cfg, series_of(cfg), out)
    G.save(case, cfg, out)


def run_fd(case, per_variable=4, h=5e-3, **overrides):
    """Central differences of the reference's ``cost`` at ``per_variable`` coordinates of every variable, by the method
    of ``make_classifier_golden.run_fd``.  No perturbation may move the arg-max over time of any ``temporal_states``
    column: the cost would have a kink between the two evaluations."""
    cfg = dict(DEFAULT, **overrides)
    series = series_of(cfg)
    ds = G.dataset(series)
    bump = {}

    def factory(name, shape, np_dtype, initializer):
        value = G.variable_factory(name, shape, np_dtype, initializer)
        if name in bump:
            idx, delta = bump[name]
            value = value.copy()
            value.reshape(-1)[idx] += np.asarray(delta, value.dtype)
        return value

    def loss():
        G.fresh_graph()
        _, enc, _, dec, parts = build(cfg)
        with tf_eager.feeding(G.feed(parts, ds, False, inputs_of())):
            where = np.argmax(enc.temporal_states.numpy(), axis=1)
            return float(dec.cost.numpy()), where
    tf_eager.VARIABLE_FACTORY = factory
    try:
        out = {}
        forward(cfg, series, out)
        _, base = loss()
        order, params = G.variables()
        rng = np.random.default_rng(zlib.crc32(case.encode()))
        names, index, value = [], [], []
        for name in order:
            v = params[name]
            if v.dtype.kind != "f" or v.size == 0:
                continue
            for i in rng.choice(v.size, size=min(per_variable, v.size), replace=False):
                bump.clear()
                bump[name] = (int(i), +h)
                up, where_up = loss()
                bump[name] = (int(i), -h)
                down, where_down = loss()
                assert np.array_equal(where_up, base) and np.array_equal(where_down, base), \
                    "{}: perturbing {}[{}] moves a maximum over time; choose another seed".format(case, name, i)
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
        tf_eager.VARIABLE_FACTORY = G.variable_factory
    G.save(case, cfg, out)


def write_signatures():
    """tests/golden/convs2s_signatures.json: the constructor parameters of the reference's class."""
    sys.path.insert(0, os.path.join(G.REPO))
    from tests.test_reference_signatures import read_reference_parameters
    path = "encoders/facebook_conv.py"
    lists = {path: {"SentenceEncoder": read_reference_parameters(path, "SentenceEncoder")}}
    with open(os.path.join(HERE, "convs2s_signatures.json"), "w", encoding="utf-8") as handle:
        json.dump(lists, handle, indent=1, sort_keys=True)
        handle.write("\n")


def write_bundle():
    """tests/golden/reference_tests_convs2s.tar.gz: tests/bpe.ini and the two word lists it names, byte for byte (the
    corpora it names are in reference_tests.tar.gz)."""
    import gzip
    import io
    import tarfile
    raw = io.BytesIO()
    with tarfile.open(fileobj=raw, mode="w", format=tarfile.GNU_FORMAT) as tar:
        for rel in ("tests/bpe.ini", "tests/data/merges_100.bpe", "tests/data/bpe_vocab.tsv"):
            with open(os.path.join(G.REFERENCE, rel), "rb") as handle:
                data = handle.read()
            info = tarfile.TarInfo(rel)
            info.size, info.mode, info.mtime = len(data), 0o644, 0
            tar.addfile(info, io.BytesIO(data))
    with open(os.path.join(HERE, "reference_tests_convs2s.tar.gz"), "wb") as handle:
        with gzip.GzipFile(fileobj=handle, mode="wb", mtime=0, filename="") as gz:
            gz.write(raw.getvalue())


CASES = collections.OrderedDict([
    ("convs2s_k5", lambda c: run_forward(c)),
    ("convs2s_k4_one_layer", lambda c: run_forward(c, kernel_width=4, encoder_layers=1, conv_features=7, seed=42)),
    ("convs2s_k3_truncated", lambda c: run_forward(c, kernel_width=3, encoder_layers=3, max_length=5, seed=43)),
    ("convs2s_classifier", lambda c: run_forward(c, head="classifier", layers=[8], seed=44)),
    ("fd_gradients_convs2s", lambda c: run_fd(c, head="classifier", layers=[8], seed=45)),
])


if __name__ == "__main__":
    for name in (sys.argv[1:] or list(CASES)):
        CASES[name](name)
    if not sys.argv[1:]:
        write_signatures()
        write_bundle()
