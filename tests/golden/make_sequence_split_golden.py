"""Generate ``tests/golden/sequence_split/*.npz``: SequenceSplitter run by the REFERENCE'S OWN Python.

Runs only where the reference tree is (nothing at test time needs it).  It imports the helpers of
``make_reference_exec_golden.py`` -- the NumPy-eager TensorFlow stand-in (which has ``tf.layers.dense``), the name-seeded
variable factory, ``save`` -- and ``neuralmonkey.model.sequence_split`` UNMODIFIED.  The fixtures have the layout of
``tests/golden/ref_exec`` (``cfg``, ``var_order``, ``p/<variable>``, ``in/*``, ``out/*``) in a directory of their own.

    python tests/golden/make_sequence_split_golden.py            # all cases

Every batch: 3 ragged sentences over 11 source words, embeddings of 12, so the variable names and shapes the reference
creates for the optional projection, one forward pass, the mask and ``lengths`` of the longer sequence are on record."""
import collections
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_exec_golden as G  # noqa: E402  pylint: disable=wrong-import-position

tf, tf_eager = G.tf, G.tf_eager
G.OUT = os.path.join(HERE, "sequence_split")

DEFAULT = dict(src_vocab=11, emb=12, factor=2, projection_size=None, activation=None, seed=51, batch=3)


def run(case, **overrides):
    from neuralmonkey.model.sequence import EmbeddedSequence
    from neuralmonkey.model.sequence_split import SequenceSplitter
    cfg = dict(DEFAULT, **overrides)
    rng = np.random.default_rng(cfg["seed"])
    series = {"source": G.sentences(rng, cfg["batch"], cfg["src_vocab"], 1, 5)}
    series["source"][-1] = series["source"][-1][:1]
    G.fresh_graph()
    seq = EmbeddedSequence(name="input", vocabulary=G.make_vocab(cfg["src_vocab"]), data_id="source",
                           embedding_size=cfg["emb"])
    act = {None: None, "relu": tf.nn.relu, "tanh": tf.tanh}[cfg["activation"]]
    split = SequenceSplitter(name="splitter", parent=seq, factor=cfg["factor"],
                             projection_size=cfg["projection_size"], projection_activation=act)
    parts = [seq, split]
    out = {}
    with tf_eager.feeding(G.feed(parts, G.dataset(series), False, G.string_inputs("source"))):
        out["in/src_ids"] = seq.inputs.numpy()
        out["in/parent_states"] = seq.temporal_states.numpy()
        out["in/parent_mask"] = seq.temporal_mask.numpy()
        out["out/temporal_states"] = split.temporal_states.numpy()
        out["out/temporal_mask"] = split.temporal_mask.numpy()
        out["out/lengths"] = split.lengths.numpy()
        out["out/dimension"] = np.asarray(split.dimension)
        out["out/dependencies"] = np.asarray(split.dependencies)
    G.save(case, cfg, out)


CASES = collections.OrderedDict([
    ("split_plain", lambda c: run(c, factor=3)),
    ("split_projected_relu", lambda c: run(c, factor=2, projection_size=8, activation="relu", seed=52)),
    ("split_projected_tanh", lambda c: run(c, factor=4, projection_size=16, activation="tanh", seed=53)),
    ("split_projected_linear", lambda c: run(c, factor=2, projection_size=6, seed=54)),
])


if __name__ == "__main__":
    for name in (sys.argv[1:] or list(CASES)):
        CASES[name](name)
