"""Generate ``tests/golden/classifier/*.npz``: the sentence-level heads run by the REFERENCE'S OWN Python.

Runs only where the reference tree is (nothing at test time needs it).  It imports the helpers of
``make_reference_exec_golden.py`` -- the NumPy-eager TensorFlow stand-in, the name-seeded variable factory, ``save`` --
and ``neuralmonkey.encoders.pooling`` / ``encoders.attentive`` / ``decoders.classifier`` /
``decoders.sequence_regressor`` / ``runners.{runner,logits_runner,regression_runner}`` UNMODIFIED.  The fixtures have the
layout of ``tests/golden/ref_exec`` (``cfg``, ``p/<variable>``, ``in/*``, ``out/*``) but live in a directory of their
own: the contents of ``ref_exec`` are pinned by tests/test_reference_exec_regen.py.

The stand-in has no ``tf.assert_greater`` (SequenceMaxPooling, pooling.py:49); this file supplies one that raises as
TensorFlow's does.  The stand-in computes no gradients, so the gradient-reversal views have no fixture.

    python tests/golden/make_classifier_golden.py            # all cases
    python tests/golden/make_classifier_golden.py max_pooling

Every batch: 5 ragged sentences over 17 source words, one of a single word, one with an unknown word; embeddings of 6,
a bidirectional GRU of 5 (SentenceEncoder); 6 classes.
"""
import collections
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_exec_golden as G  # noqa: E402  pylint: disable=wrong-import-position

tf, tf_eager = G.tf, G.tf_eager
G.OUT = os.path.join(HERE, "classifier")


def assert_greater(x, y, *_args, **_kwargs):
    """tf.assert_greater for the eager stand-in: checked at once."""
    xv = x.numpy() if hasattr(x, "numpy") else np.asarray(x)
    yv = y.numpy() if hasattr(y, "numpy") else np.asarray(y)
    if not np.all(xv > yv):
        raise ValueError("assert_greater failed: {} > {}".format(xv, yv))
    return None


tf.assert_greater = assert_greater

LENGTHS = [4, 7, 3, 6, 1]

DEFAULT = dict(src_vocab=17, cls_vocab=6, emb=6, rnn=5, encoders=["max"], head=None, hidden_size=7, num_heads=3,
               state_proj_size=None, output_size=None, layers=[], activation="relu", dimension=1, seed=21, batch=5)


def build(cfg):
    from neuralmonkey.decoders.classifier import Classifier
    from neuralmonkey.decoders.sequence_regressor import SequenceRegressor
    from neuralmonkey.encoders.attentive import AttentiveEncoder
    from neuralmonkey.encoders.pooling import SequenceAveragePooling, SequenceMaxPooling
    from neuralmonkey.encoders.recurrent import SentenceEncoder
    sv, cv = G.make_vocab(cfg["src_vocab"]), G.make_vocab(cfg["cls_vocab"])
    enc = SentenceEncoder(name="encoder", vocabulary=sv, data_id="source", embedding_size=cfg["emb"],
                          rnn_size=cfg["rnn"])
    parts, readers = [enc.input_sequence, enc], collections.OrderedDict()
    for kind in cfg["encoders"]:
        if kind == "max":
            readers[kind] = SequenceMaxPooling(name="encoder_max", input_sequence=enc)
        elif kind == "avg":
            readers[kind] = SequenceAveragePooling(name="encoder_avg", input_sequence=enc)
        else:
            readers[kind] = AttentiveEncoder(name="encoder_att", input_sequence=enc, hidden_size=cfg["hidden_size"],
                                             num_heads=cfg["num_heads"], output_size=cfg["output_size"],
                                             state_proj_size=cfg["state_proj_size"])
    parts += list(readers.values())
    act = {"relu": tf.nn.relu, "tanh": tf.tanh}[cfg["activation"]]
    dec = None
    if cfg["head"] == "classifier":
        dec = Classifier(name="classifier", encoders=list(readers.values()), vocabulary=cv, data_id="target",
                         layers=cfg["layers"], activation_fn=act, dropout_keep_prob=1.0)
    elif cfg["head"] == "regressor":
        dec = SequenceRegressor(name="regressor", encoders=list(readers.values()), data_id="target",
                                layers=cfg["layers"], activation_fn=act, dimension=cfg["dimension"])
    if dec is not None:
        parts.append(dec)
    return enc, readers, dec, parts


def series_of(cfg):
    """Source sentences of ``LENGTHS`` words (sentence 0 carries an unknown word, the last has one word) and one
    target per sentence: a class word (sentence 0: an unknown one), or a row of floats whose first value counts."""
    rng = np.random.default_rng(cfg["seed"])
    src = [["w{}".format(int(rng.integers(0, cfg["src_vocab"]))) for _ in range(n)] for n in LENGTHS]
    src[0][1] = "never-seen"
    if cfg["head"] == "regressor":
        tgt = [np.asarray([rng.normal(0, 1.5), 99.0], np.float32) for _ in src]
    else:
        tgt = [["w{}".format(int(rng.integers(0, cfg["cls_vocab"])))] for _ in src]
        tgt[0] = ["never-seen"]
        tgt[2] = tgt[2] + ["w1"]                                # only the first token of a target counts
    return {"source": src, "target": tgt}


def inputs_of(cfg):
    inputs = G.string_inputs("source")
    if cfg["head"] == "regressor":
        inputs["target"] = tf.placeholder(tf.float32, [None], "target")
    else:
        inputs["target"] = tf.placeholder(tf.string, [None], "target")
    return inputs


def padded_argmax(states, mask):
    """Position of every column's maximum of pooling.py:50's padded input."""
    m = mask[:, :, None]
    return np.argmax(states * m + np.float32(1e-15) * (1 - m), axis=1)


def forward(cfg, series, out):
    G.fresh_graph()
    enc, readers, dec, parts = build(cfg)
    ds = G.dataset(series)
    with tf_eager.feeding(G.feed(parts, ds, False, inputs_of(cfg))):
        out["in/src_tokens"] = enc.input_sequence.input_factors[0].numpy()
        out["in/src_ids"] = enc.input_sequence.inputs.numpy()
        out["out/enc_states"] = enc.temporal_states.numpy()
        out["out/enc_mask"] = enc.temporal_mask.numpy()
        for kind, part in readers.items():
            out["out/{}_output".format(kind)] = part.output.numpy()
            if kind == "att":
                out["out/att_weights"] = part.attention_weights.numpy()
                out["out/att_temporal_states"] = part.temporal_states.numpy()
                out["out/att_temporal_mask"] = part.temporal_mask.numpy()
        if cfg["head"] == "classifier":
            from neuralmonkey.runners.logits_runner import LogitsRunner
            from neuralmonkey.runners.runner import GreedyRunner
            out["in/tgt_tokens"] = np.asarray(dec.targets.numpy())
            out["in/tgt_ids"] = dec.gt_inputs.numpy()
            out["out/decoded_seq"] = dec.decoded_seq.numpy()
            out["out/decoded_logits"] = dec.decoded_logits.numpy()
            out["out/runtime_logprobs"] = dec.runtime_logprobs.numpy()
            out["out/cost"] = dec.cost.numpy()
            for tag, runner in (("greedy", GreedyRunner(output_series="cls", decoder=dec)),
                                ("logits", LogitsRunner(output_series="dist", decoder=dec)),
                                ("logits_raw_pick0", LogitsRunner(output_series="dist", decoder=dec, normalize=False,
                                                                  pick_index=0)),
                                ("logits_pick", LogitsRunner(output_series="dist", decoder=dec, pick_value="w2"))):
                ex = runner.get_executable(compute_losses=True, summaries=False, num_sessions=1)
                fetches, _ = ex.next_to_execute()
                ex.collect_results([G.to_numpy(fetches)])
                series_name = runner.output_series
                out["out/runner_{}".format(tag)] = np.asarray([G.joined(s) for s in ex.result.outputs[series_name]])
                out["out/runner_{}_losses".format(tag)] = np.asarray(
                    [ex.result.losses[k] for k in sorted(ex.result.losses)], np.float32)
        elif cfg["head"] == "regressor":
            from neuralmonkey.runners.regression_runner import RegressionRunner
            out["in/targets"] = np.asarray(dec.train_inputs.numpy(), np.float32)
            out["out/predictions"] = dec.predictions.numpy()
            out["out/cost"] = dec.cost.numpy()
            runner = RegressionRunner(output_series="reg", decoder=dec)
            ex = runner.get_executable(compute_losses=True, summaries=False, num_sessions=1)
            fetches, _ = ex.next_to_execute()
            ex.collect_results([G.to_numpy(fetches)])
            out["out/runner_predictions"] = np.asarray(ex.result.outputs["reg"], np.float32)
            out["out/runner_mse"] = np.asarray(ex.result.losses["reg/mse"], np.float32)
    return dec, parts


def run_forward(case, **overrides):
    cfg = dict(DEFAULT, **overrides)
    out = {}
    forward(cfg, series_of(cfg), out)
    G.save(case, cfg, out)


def run_fd(case, per_variable=4, h=5e-3, **overrides):
    """Central differences of the reference's ``cost`` at ``per_variable`` coordinates of every variable, by the method
    of ``make_labeler_golden.run_fd`` (the graph rebuilt for each evaluation).  No perturbation may change which
    position holds the maximum of a max-pooled column: the cost would have a kink between the two evaluations."""
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
        enc, _, dec, parts = build(cfg)
        with tf_eager.feeding(G.feed(parts, ds, False, inputs_of(cfg))):
            where = padded_argmax(enc.temporal_states.numpy(), enc.temporal_mask.numpy())
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
                if "max" in cfg["encoders"]:
                    assert np.array_equal(where_up, base) and np.array_equal(where_down, base), \
                        "{}: perturbing {}[{}] moves a pooled maximum; choose another seed".format(case, name, i)
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


CASES = collections.OrderedDict([
    ("max_pooling", lambda c: run_forward(c, encoders=["max"])),
    ("average_pooling", lambda c: run_forward(c, encoders=["avg"], seed=22)),
    ("attentive_plain", lambda c: run_forward(c, encoders=["att"], seed=23)),
    ("attentive_projected", lambda c: run_forward(c, encoders=["att"], state_proj_size=4, output_size=9, seed=24)),
    ("classifier_attentive_maxpool", lambda c: run_forward(c, encoders=["att", "max"], head="classifier",
                                                           layers=[8, 5], output_size=9, seed=25)),
    ("classifier_no_layers", lambda c: run_forward(c, encoders=["avg"], head="classifier", seed=26)),
    ("regressor_two_dimensions", lambda c: run_forward(c, encoders=["max"], head="regressor", layers=[7], dimension=2,
                                                       seed=27)),
    ("fd_gradients_classifier", lambda c: run_fd(c, encoders=["att", "max"], head="classifier", layers=[8],
                                                 activation="tanh", state_proj_size=4, output_size=9, seed=28)),
    ("fd_gradients_regressor", lambda c: run_fd(c, encoders=["avg", "max"], head="regressor", layers=[7],
                                                activation="tanh", dimension=2, seed=32)),
])


if __name__ == "__main__":
    for name in (sys.argv[1:] or list(CASES)):
        CASES[name](name)
