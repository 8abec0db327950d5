"""Generate ``tests/golden/self_critical/*.npz``, ``tests/golden/reference_tests_self_critical.tar.gz`` and
``tests/golden/self_critical_signatures.json``: self-critical training as the REFERENCE'S OWN Python computes it.

Runs only where the reference tree is (nothing at test time needs it).  It imports the helpers of
``make_reference_exec_golden.py`` -- the NumPy-eager TensorFlow stand-in, the name-seeded variable factory, the RNN
encoder-decoder builder, ``save`` -- and ``neuralmonkey.trainers.self_critical_objective`` UNMODIFIED.

The stand-in's ``tf.py_func`` returns a list whatever ``Tout`` is; TensorFlow returns ONE tensor for a ``Tout`` that is
no list (python/ops/script_ops.py), which is what the objective subtracts.  This file supplies that one.

    python tests/golden/make_self_critical_golden.py                 # everything
    python tests/golden/make_self_critical_golden.py rewards          # one case

``rewards``                       sentence_bleu / sentence_gleu on fixed token arrays (random ones over small
                                  vocabularies, and hand-made columns around the end token)
``self_critical_gru``             5 ragged sentences, 8 target words, a GRU decoder of 6 with one Bahdanau attention over a
                                  bidirectional GRU encoder of 5 (embeddings of 5), keep 1.0, max_output_len 8: both argmax
                                  arrays, both reward vectors, the runtime mask and the loss
``fd_gradients_self_critical``    central differences of that loss at h = 5e-3.  The loss is piecewise smooth: a
                                  perturbation that changes a decoded symbol (or a reward) puts a jump between the two
                                  evaluations, so a coordinate is recorded only where both perturbed runs decode what the
                                  unperturbed run decodes and earn its rewards.
"""
import collections
import gzip
import io
import json
import os
import sys
import tarfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_exec_golden as G  # noqa: E402  pylint: disable=wrong-import-position

tf, tf_eager = G.tf, G.tf_eager
G.OUT = os.path.join(HERE, "self_critical")


def py_func(func, inp, Tout, stateful=True, name=None):     # noqa: N803  pylint: disable=invalid-name,unused-argument
    """tf.py_func for the eager stand-in: run at once; one tensor for a single ``Tout``, a list for a list."""
    out = func(*[i.numpy() if hasattr(i, "numpy") else np.asarray(i) for i in inp])
    if isinstance(Tout, (list, tuple)):
        return [tf_eager.Tensor(np.asarray(o)) for o in out]
    return tf_eager.Tensor(np.asarray(out))


tf.py_func = py_func

END = 2
CONFIG = dict(G.RNN_DEFAULT, src_vocab=17, tgt_vocab=8, emb=5, rnn_size=6, max_output_len=8, seed=43, batch=5,
              reward="sentence_bleu")


# ---- rewards ---------------------------------------------------------------------------------------------------------------
def reward_inputs():
    """name -> (references [T_ref, B], hypotheses [T_hyp, B]), int64 as tf.argmax gives them."""
    cases = collections.OrderedDict()
    rng = np.random.default_rng(20)
    for bsz in (5, 67):
        for t_ref, t_hyp in ((7, 9), (1, 3), (70, 130)):
            # vocabularies of 3 to 8 words (the end token among them): n-grams repeat, so the clipping matters
            width = rng.integers(3, 9, size=bsz)
            ref = (rng.integers(0, 1 << 30, (t_ref, bsz)) % width).astype(np.int64)
            hyp = (rng.integers(0, 1 << 30, (t_hyp, bsz)) % width).astype(np.int64)
            if t_ref == 70:                       # long sentences: few end tokens, or every sentence ends at once
                ref[ref == END] = np.where(rng.random(int((ref == END).sum())) < 0.9, 1, END)
                hyp[hyp == END] = np.where(rng.random(int((hyp == END).sum())) < 0.9, 1, END)
            cases["random_b{}_r{}_h{}".format(bsz, t_ref, t_hyp)] = (ref, hyp)
    base = [4, 5, 4, 5, 6, 3]
    columns = [
        ([4, 5, 4, 5, 6, 3], [END, 4, 5, 4, 5, 6]),           # end token at index 0: no unigram, the 2-grams go on
        ([4, 5, 4, 5, 6, 3], [4, END, 5, 4, 5, 6]),           # ... at index 1
        ([4, 5, 4, 5, 6, 3], [4, 5, END, 4, 5, 6]),           # ... at index 2
        ([END, 4, 5, 4, 5, 6], [4, 5, 4, 5, 6, 3]),           # ... in the reference
        ([4, END, END, 5, 4, 5], [4, 5, END, END, 4, 5]),
        ([4, 5, 4, 5, 6, 3], [4, 5, 4, 5, 6, 3]),             # no end token; hypothesis equal to the reference
        ([4, 5, 4, 5, END, 0], [4, 5, 4, 5, END, 0]),         # equal, with an end token
        ([4, 5, 4, 5, 6, 3], [7, 8, 7, 8, 9, 9]),             # nothing in common
        ([4, 4, 5, 6, 3, 3], [4, 4, 4, 4, 4, 4]),             # clipping: two of six
        ([4, 5, 6, END, 0, 0], [4, END, 0, 0, 0, 0]),         # brevity penalty
        ([4, 5, 6, END, 0, 0], [4, 5, 6, 7, 8, END]),
        (base, [0, 0, 0, 0, 0, 0]),
    ]
    cases["hand_made"] = (np.asarray([c[0] for c in columns], np.int64).T.copy(),
                          np.asarray([c[1] for c in columns], np.int64).T.copy())
    return cases


def run_rewards(case):
    from neuralmonkey.trainers import self_critical_objective as R
    out = {}
    for name, (ref, hyp) in reward_inputs().items():
        out[name + "/ref"], out[name + "/hyp"] = ref.astype(np.int32), hyp.astype(np.int32)
        out[name + "/bleu"] = R.sentence_bleu(ref, hyp)
        ok = np.ones(ref.shape[1], bool)
        gleu = np.zeros(ref.shape[1], np.float32)
        for b in range(ref.shape[1]):             # (the reference asserts where a sentence has no n-gram at all)
            try:
                with np.errstate(all="ignore"):
                    gleu[b] = R.sentence_gleu(ref[:, b:b + 1], hyp[:, b:b + 1])[0]
            except AssertionError:
                ok[b] = False
        out[name + "/gleu"], out[name + "/gleu_defined"] = gleu, ok
    os.makedirs(G.OUT, exist_ok=True)
    path = os.path.join(G.OUT, case + ".npz")
    np.savez_compressed(path, **out)
    print("{:28s} {:4d} arrays {:8d} bytes".format(case, len(out), os.path.getsize(path)))


# ---- the objective on a small model ------------------------------------------------------------------------------------------
def evaluate(cfg, ds, inputs):
    """One run of the reference's graph: everything the fixture keeps."""
    from neuralmonkey.trainers import self_critical_objective as R
    G.fresh_graph()
    enc, _, dec, parts = G.build_rnn(cfg)
    objective = R.SelfCriticalObjective(dec, getattr(R, cfg["reward"]))
    got = {}
    with tf_eager.feeding(G.feed(parts, ds, False, inputs)):
        got["in/src_tokens"] = enc.input_sequence.input_factors[0].numpy()
        got["in/src_ids"] = enc.input_sequence.inputs.numpy()
        got["in/tgt_tokens"] = dec.train_tokens.numpy()
        got["in/tgt_ids"] = dec.train_inputs.numpy()                          # time-major [T, B]
        train_logits, runtime_logits = dec.train_logits.numpy(), dec.runtime_logits.numpy()
        got["out/train_logits"], got["out/runtime_logits"] = train_logits, runtime_logits
        got["out/train_argmax"] = np.argmax(train_logits, axis=2).astype(np.int32)
        got["out/runtime_argmax"] = np.argmax(runtime_logits, axis=2).astype(np.int32)
        got["out/runtime_mask"] = np.asarray(dec.runtime_mask.numpy(), np.float32)
        reward = getattr(R, cfg["reward"])
        got["out/train_reward"] = reward(got["in/tgt_ids"], got["out/train_argmax"])
        got["out/runtime_reward"] = reward(got["in/tgt_ids"], got["out/runtime_argmax"])
        got["out/loss"] = np.asarray(objective.loss.numpy(), np.float64)
        got["out/name"] = np.asarray(objective.name)
    return got


def check_interesting(got):
    diff = got["out/runtime_reward"] - got["out/train_reward"]
    assert (diff != 0).sum() >= 3 and (diff > 0).any() and (diff < 0).any(), diff


def run_forward(case):
    cfg = dict(CONFIG)
    ds = G.dataset(G.rnn_series(cfg))
    got = evaluate(cfg, ds, G.string_inputs("source", "target"))
    check_interesting(got)
    G.save(case, cfg, got)


def run_fd(case, per_variable=5, h=5e-3):
    cfg = dict(CONFIG)
    ds = G.dataset(G.rnn_series(cfg))
    inputs = G.string_inputs("source", "target")
    bump = {}

    def factory(name, shape, np_dtype, initializer):
        value = G.variable_factory(name, shape, np_dtype, initializer)
        if name in bump:
            idx, delta = bump[name]
            value = value.copy()
            value.reshape(-1)[idx] += np.asarray(delta, value.dtype)
        return value

    def same_decoding(a, b):
        return all(np.array_equal(a[k], b[k]) for k in ("out/train_argmax", "out/runtime_argmax", "out/train_reward",
                                                         "out/runtime_reward", "out/runtime_mask"))
    tf_eager.VARIABLE_FACTORY = factory
    try:
        base = evaluate(cfg, ds, inputs)
        check_interesting(base)
        order, params = G.variables()
        rng = np.random.default_rng(zlib.crc32(case.encode()))
        names, index, value, tried = [], [], [], 0
        for name in order:
            v = params[name]
            if v.dtype.kind != "f" or v.size == 0:
                continue
            kept = 0
            for i in rng.choice(v.size, size=min(per_variable, v.size), replace=False):
                tried += 1
                bump.clear()
                bump[name] = (int(i), +h)
                up = evaluate(cfg, ds, inputs)
                bump[name] = (int(i), -h)
                down = evaluate(cfg, ds, inputs)
                if not (same_decoding(up, base) and same_decoding(down, base)):
                    continue                      # a jump between the two evaluations: the difference means nothing
                names.append(name)
                index.append(int(i))
                value.append((float(up["out/loss"]) - float(down["out/loss"])) / (2.0 * h))
                kept += 1
            assert kept >= min(3, v.size), "{}: {} of {} coordinates kept; choose another seed".format(name, kept, v.size)
        assert 4 * (tried - len(names)) <= tried, "{} of {} coordinates dropped".format(tried - len(names), tried)
        bump.clear()
        out = evaluate(cfg, ds, inputs)               # leave the unperturbed variables in the store for save()
        out["fd/names"] = np.asarray(names)
        out["fd/index"] = np.asarray(index, np.int64)
        out["fd/value"] = np.asarray(value, np.float64)
        out["fd/h"] = np.asarray(h)
        out["fd/tried"] = np.asarray(tried)
    finally:
        tf_eager.VARIABLE_FACTORY = G.variable_factory
    G.save(case, cfg, out)


# ---- the reference's configuration and constructor -----------------------------------------------------------------------------
SIGNATURES = os.path.join(HERE, "self_critical_signatures.json")
BUNDLE = os.path.join(HERE, "reference_tests_self_critical.tar.gz")


def signatures():
    sys.path.insert(0, os.path.join(G.REPO))
    from tests.test_reference_signatures import read_reference_parameters
    path = "trainers/self_critical_objective.py"
    return {path: {"SelfCriticalObjective": read_reference_parameters(path, "SelfCriticalObjective")}}


def write_bundle():
    """tests/self-critical.ini byte for byte (every data file it names is in reference_tests.tar.gz already) and the
    constructor's parameters, as a JSON file beside it and inside the archive."""
    text = json.dumps(signatures(), indent=1, sort_keys=True) + "\n"
    with open(SIGNATURES, "w", encoding="utf-8") as handle:
        handle.write(text)
    with open(os.path.join(G.REFERENCE, "tests", "self-critical.ini"), "rb") as handle:
        ini = handle.read()
    raw = io.BytesIO()
    with tarfile.open(fileobj=raw, mode="w", format=tarfile.GNU_FORMAT) as tar:
        for rel, data in (("tests/self-critical.ini", ini), ("self_critical_signatures.json", text.encode())):
            info = tarfile.TarInfo(rel)
            info.size, info.mode, info.mtime = len(data), 0o644, 0
            tar.addfile(info, io.BytesIO(data))
    with open(BUNDLE, "wb") as handle:
        with gzip.GzipFile(fileobj=handle, mode="wb", mtime=0, filename="") as gz:
            gz.write(raw.getvalue())
    print(BUNDLE, os.path.getsize(BUNDLE))


CASES = collections.OrderedDict([
    ("rewards", run_rewards),
    ("self_critical_gru", run_forward),
    ("fd_gradients_self_critical", run_fd),
])


if __name__ == "__main__":
    for name_ in (sys.argv[1:] or list(CASES)):
        CASES[name_](name_)
    if not sys.argv[1:]:
        write_bundle()
