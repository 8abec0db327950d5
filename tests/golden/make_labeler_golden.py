"""Generate ``tests/golden/labeler/*.npz``: the sequence-labelling heads run by the REFERENCE'S OWN Python.

Runs only where the reference tree is (nothing at test time needs it).  It imports the helpers of
``make_reference_exec_golden.py`` -- the NumPy-eager TensorFlow stand-in, the name-seeded variable factory, ``save`` --
and ``neuralmonkey.decoders.sequence_labeler`` / ``neuralmonkey.runners.label_runner`` UNMODIFIED.  The fixtures have the
layout of ``tests/golden/ref_exec`` (``cfg``, ``p/<variable>``, ``in/*``, ``out/*``) but live in a directory of their
own: the contents of ``ref_exec`` are pinned by tests/test_reference_exec_regen.py.

    python tests/golden/make_labeler_golden.py            # all cases
    python tests/golden/make_labeler_golden.py labeler_plain

Every batch: 5 ragged sentences over 17 source words and 9 tags, one of a single word, one with an out-of-vocabulary
tag (and source word); embeddings of 6, a bidirectional GRU of 5.
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
G.OUT = os.path.join(HERE, "labeler")

DEFAULT = dict(src_vocab=17, tag_vocab=9, emb=6, encoder="gru", rnn=5, second_encoder=None, head="sequence",
               hidden_dim=None, activation="relu", train_embeddings=True, max_output_len=None, add_start_symbol=False,
               add_end_symbol=False, ff=10, depth=2, heads=2, seed=11, batch=5)


def build(cfg):
    from neuralmonkey.decoders.sequence_labeler import EmbeddingsLabeler, SequenceLabeler
    from neuralmonkey.encoders.recurrent import RecurrentEncoder
    from neuralmonkey.encoders.transformer import TransformerEncoder
    from neuralmonkey.model.sequence import EmbeddedSequence
    sv, tv = G.make_vocab(cfg["src_vocab"]), G.make_vocab(cfg["tag_vocab"])
    seq = EmbeddedSequence(name="encoder_input", vocabulary=sv, data_id="source", embedding_size=cfg["emb"])
    if cfg["encoder"] == "gru":
        enc = RecurrentEncoder(name="encoder", input_sequence=seq, rnn_layers=[(cfg["rnn"], "bidirectional", "GRU")])
    else:
        enc = TransformerEncoder(name="encoder", input_sequence=seq, ff_hidden_size=cfg["ff"], depth=cfg["depth"],
                                 n_heads=cfg["heads"])
    encoders, parts = [enc], [seq, enc]
    if cfg["second_encoder"] is not None:            # a second encoder over the SAME sequence: equal temporal masks
        enc2 = RecurrentEncoder(name="encoder2", input_sequence=seq,
                                rnn_layers=[(cfg["second_encoder"], "forward", "GRU")])
        encoders.append(enc2)
        parts.append(enc2)
    act = {"relu": tf.nn.relu, "tanh": tf.tanh}[cfg["activation"]]
    common = dict(data_id="tags", max_output_len=cfg["max_output_len"], hidden_dim=cfg["hidden_dim"], activation=act,
                  add_start_symbol=cfg["add_start_symbol"], add_end_symbol=cfg["add_end_symbol"])
    if cfg["head"] == "sequence":
        dec = SequenceLabeler(name="tagger", encoders=encoders, vocabulary=tv, **common)
    else:
        dec = EmbeddingsLabeler(name="tagger", encoders=encoders, embedded_sequence=seq,
                                train_embeddings=cfg["train_embeddings"], **common)
    return seq, encoders, dec, parts + [dec]


def series_of(cfg):
    """Source sentences and one tag per word; sentence 0 carries an unknown word and an unknown tag, the last sentence
    has one word.  An EmbeddingsLabeler's tags are words of the source vocabulary with holes (<pad>), as the masked
    language model of tests/bert.ini feeds them."""
    rng = np.random.default_rng(cfg["seed"])
    src = G.sentences(rng, cfg["batch"], cfg["src_vocab"], 2, 7, oov_every=2)
    src[-1] = src[-1][:1]
    src[1] = (src[1] * 7)[:7]
    tags = []
    for i, sent in enumerate(src):
        if cfg["head"] == "sequence":
            row = ["w{}".format(int(rng.integers(0, cfg["tag_vocab"]))) for _ in sent]
        else:
            row = [w if rng.random() < 0.6 else "<pad>" for w in sent]
            if i == 1:
                row = list(sent)
        if i == 0:
            row[-1] = "never-seen"
        tags.append(row)
    return {"source": src, "tags": tags}


def forward(cfg, series, out):
    from neuralmonkey.runners.label_runner import LabelRunner
    G.fresh_graph()
    seq, encoders, dec, parts = build(cfg)
    inputs = G.string_inputs("source", "tags")
    ds = G.dataset(series)
    with tf_eager.feeding(G.feed(parts, ds, False, inputs)):
        out["in/src_tokens"] = seq.input_factors[0].numpy()
        out["in/src_ids"] = seq.inputs.numpy()
        out["in/tgt_tokens"] = dec.target_tokens.numpy()
        out["in/tgt_ids"] = dec.train_targets.numpy()
        for i, enc in enumerate(encoders):
            out["out/enc{}_states".format(i)] = enc.temporal_states.numpy()
        out["out/input_mask"] = dec.input_mask.numpy()
        out["out/states"] = dec.states.numpy()
        out["out/logits"] = dec.logits.numpy()
        out["out/logprobs"] = dec.logprobs.numpy()
        out["out/decoded"] = dec.decoded.numpy()
        out["out/train_mask"] = dec.train_mask.numpy()
        out["out/train_xents"] = dec.train_xents.numpy()
        out["out/cost"] = dec.cost.numpy()
        runner = LabelRunner(output_series="tags", decoder=dec)
        ex = runner.get_executable(compute_losses=True, summaries=False, num_sessions=1)
        fetches, _ = ex.next_to_execute()
        ex.collect_results([G.to_numpy(fetches)])
        out["out/runner_sentences"] = np.asarray([G.joined(s) for s in ex.result.outputs["tags"]])
        out["out/runner_loss"] = np.asarray(ex.result.losses["tags/loss"], np.float32)
    return dec, parts


def run_forward(case, **overrides):
    cfg = dict(DEFAULT, **overrides)
    out = {}
    forward(cfg, series_of(cfg), out)
    G.save(case, cfg, out)


def run_feed(case, **overrides):
    """feed_dict alone: pad_batch with max_output_len / add_start_symbol / add_end_symbol (vocabulary.py:331-354)."""
    cfg = dict(DEFAULT, **overrides)
    series = series_of(cfg)
    G.fresh_graph()
    _, _, dec, parts = build(cfg)
    with tf_eager.feeding(G.feed(parts, G.dataset(series), False, G.string_inputs("source", "tags"))):
        out = {"in/tags": np.asarray([" ".join(s) for s in series["tags"]]),
               "in/tgt_tokens": dec.target_tokens.numpy(), "in/tgt_ids": dec.train_targets.numpy(),
               "out/train_mask": dec.train_mask.numpy()}
    G.save(case, cfg, out)


def run_fd(case, per_variable=4, h=5e-3, **overrides):
    """Central differences of the reference's ``cost`` at ``per_variable`` coordinates of every variable, by the method
    of ``make_reference_exec_golden.run_fd_gradients`` (the graph rebuilt for each evaluation)."""
    cfg = dict(DEFAULT, **overrides)
    series = series_of(cfg)
    ds = G.dataset(series)
    inputs = G.string_inputs("source", "tags")
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
        _, _, dec, parts = build(cfg)
        with tf_eager.feeding(G.feed(parts, ds, False, inputs)):
            return float(dec.cost.numpy())
    tf_eager.VARIABLE_FACTORY = factory
    try:
        out = {}
        forward(cfg, series, out)
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
        tf_eager.VARIABLE_FACTORY = G.variable_factory
    G.save(case, cfg, out)


CASES = collections.OrderedDict([
    ("labeler_plain", lambda c: run_forward(c)),
    ("labeler_hidden_relu", lambda c: run_forward(c, hidden_dim=7, activation="relu", seed=12)),
    ("labeler_two_encoders", lambda c: run_forward(c, second_encoder=4, seed=13)),
    ("embeddings_labeler_transformer", lambda c: run_forward(c, head="embeddings", encoder="transformer", seed=14)),
    ("embeddings_labeler_projected", lambda c: run_forward(c, head="embeddings", seed=15)),
    ("embeddings_labeler_frozen", lambda c: run_forward(c, head="embeddings", train_embeddings=False, seed=16)),
    ("labeler_feed", lambda c: run_feed(c, max_output_len=4, add_start_symbol=True, add_end_symbol=True, seed=17)),
    ("fd_gradients_labeler", lambda c: run_fd(c, hidden_dim=7, activation="tanh", seed=18)),
    ("fd_gradients_embeddings_labeler", lambda c: run_fd(c, head="embeddings", seed=19)),
])


if __name__ == "__main__":
    for name in (sys.argv[1:] or list(CASES)):
        CASES[name](name)
