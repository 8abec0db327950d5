"""Generate ``tests/golden/reinforce/*.npz``, ``tests/golden/reference_tests_rl.tar.gz`` and
``tests/golden/reinforce_signatures.json``: REINFORCE training with sentence-level feedback as the REFERENCE'S OWN Python
computes it.

Runs only where the reference tree is (nothing at test time needs it).  It imports the helpers of
``make_reference_exec_golden.py`` -- the NumPy-eager TensorFlow stand-in, the name-seeded variable factory, the RNN
encoder-decoder builder, ``save`` -- and ``neuralmonkey.trainers.rl_trainer`` and ``neuralmonkey.evaluators.{gleu,bleu}``
UNMODIFIED (the evaluators' package file imports scorers this machine does not have, so the package is entered as an
empty module whose path is the reference's directory: the three files run as they are).

What the stand-in lacks is supplied here, at run time:

``tf.multinomial``   one draw per row by Gumbel-argmax over the float32 logits from a seeded NumPy generator, RECORDED; a
                     later run may replay recorded draws instead (finite differences)
``tf.py_func``       runs at once and returns ONE tensor for a single ``Tout`` (see make_self_critical_golden.py); it keeps
                     the function it was handed -- the reference's own ``_score_with_reward_function`` -- for the
                     ``scores`` case, and may return held rewards instead (finite differences)
``tf.Variable`` / ``tf.assign_add``   the baseline's two scalars, kept by name across runs so that two consecutive runs
                     carry the counter and the sum like two session runs do
``tf.stack`` / ``tf.div``   unchanged, but what they return inside the loss is kept: the stacked rewards and sentence
                     log-probabilities (rl_trainer.py:146-147) and the baseline (:162-163)

    python tests/golden/make_reinforce_golden.py                 # everything
    python tests/golden/make_reinforce_golden.py scores           # one case

``scores``                  ``_score_with_reward_function`` with GLEUEvaluator() and BLEUEvaluator() on fixed token
                            arrays: random ones over small vocabularies and hand-made columns
``reinforce_<mode>``        the four modes of the class docstring on the model of make_self_critical_golden.py: the
                            draws, the rewards, the baseline, the sentence log-probabilities and the loss -- of two
                            consecutive runs where there is a baseline
``fd_gradients_reinforce``  central differences of the loss at h = 5e-3 in the mode of tests/rl.ini, the recorded draws
                            replayed and the rewards held: the loss is smooth in the variables then
"""
import collections
import gzip
import io
import json
import os
import sys
import tarfile
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_exec_golden as G  # noqa: E402  pylint: disable=wrong-import-position

tf, tf_eager = G.tf, G.tf_eager
G.OUT = os.path.join(HERE, "reinforce")

import neuralmonkey  # noqa: E402,F401  pylint: disable=wrong-import-position,unused-import
_PACKAGE = types.ModuleType("neuralmonkey.evaluators")
_PACKAGE.__path__ = [os.path.join(G.REFERENCE, "neuralmonkey", "evaluators")]
sys.modules["neuralmonkey.evaluators"] = _PACKAGE

END, PAD = 2, 0
CONFIG = dict(G.RNN_DEFAULT, src_vocab=17, tgt_vocab=8, emb=5, rnn_size=6, max_output_len=8, seed=43, batch=5)
MODES = collections.OrderedDict([
    ("bandit", dict(sample_size=1, subtract_baseline=True)),
    ("mrt", dict(sample_size=3, normalize=True, alpha=0.5)),
    ("google", dict(sample_size=2, temperature=2.0)),
    ("mixed", dict(sample_size=2, subtract_baseline=True, normalize=False, ce_smoothing=0.5)),      # tests/rl.ini
])

# ---- what the stand-in lacks ---------------------------------------------------------------------------------------------
RUN = {"rng": None, "replay": None, "held": None, "draws": [], "samples": [], "rewards": [], "score": None,
       "stacked": [], "divided": [], "kept": {}}


def multinomial(logits, num_samples, seed=None, name=None, output_dtype=None):     # pylint: disable=unused-argument
    assert num_samples == 1
    x = np.asarray(logits.numpy(), np.float32)
    if RUN["replay"] is not None:
        drawn = np.asarray(RUN["replay"].pop(0), np.int64)
    else:
        drawn = np.argmax(x.astype(np.float64) + RUN["rng"].gumbel(size=x.shape), axis=1).astype(np.int64)
    RUN["draws"].append(drawn)
    return tf_eager.Tensor(drawn[:, None])


def py_func(func, inp, Tout, stateful=True, name=None):     # noqa: N803  pylint: disable=invalid-name,unused-argument
    args = [i.numpy() if hasattr(i, "numpy") else np.asarray(i) for i in inp]
    RUN["score"] = func
    RUN["samples"].append((np.asarray(args[1], np.int32), np.asarray(RUN["draws"], np.int32)))
    del RUN["draws"][:]
    out = func(*args) if RUN["held"] is None else RUN["held"][len(RUN["rewards"])]
    assert not isinstance(Tout, (list, tuple))
    RUN["rewards"].append(np.asarray(out, np.float32))
    return tf_eager.Tensor(np.asarray(out))


def kept_variable(value, trainable=True, name=None):
    assert not trainable and name
    if name not in RUN["kept"]:
        RUN["kept"][name] = tf_eager.Variable(np.asarray(value, np.float32), name, trainable)
    return RUN["kept"][name]


def assign_add(ref, value, use_locking=None, name=None):     # pylint: disable=unused-argument
    current = np.asarray(ref.numpy(), np.float32)
    return ref.assign((current + np.asarray(tf_eager.Tensor(value).numpy() if not hasattr(value, "numpy")
                                             else value.numpy(), np.float32)).astype(np.float32))


def keeping(fn, into):
    def wrapped(*args, **kwargs):
        out = fn(*args, **kwargs)
        RUN[into].append(np.asarray(out.numpy()))
        return out
    return wrapped


tf.multinomial, tf.py_func, tf.Variable, tf.assign_add = multinomial, py_func, kept_variable, assign_add
tf.stack, tf.div = keeping(tf.stack, "stacked"), keeping(tf.div, "divided")


def evaluators():
    from neuralmonkey.evaluators.bleu import BLEUEvaluator
    from neuralmonkey.evaluators.gleu import GLEUEvaluator
    return collections.OrderedDict([("gleu", GLEUEvaluator), ("bleu", BLEUEvaluator)])


# ---- the objective on a small model ----------------------------------------------------------------------------------------
def evaluate(cfg, mode, ds, inputs, seed=None, replay=None, held=None, reward="gleu"):
    """One run of the reference's graph: everything the fixture keeps.  The baseline's state is whatever the runs
    before left in ``RUN["kept"]``."""
    from neuralmonkey.trainers import rl_trainer as R
    G.fresh_graph()
    enc, _, dec, parts = G.build_rnn(cfg)
    objective = R.ReinforceObjective(dec, evaluators()[reward](), **mode)
    RUN["rng"] = np.random.default_rng(seed)
    RUN["replay"] = None if replay is None else [row for sample in replay for row in sample]
    RUN["held"] = held
    for key in ("draws", "samples", "rewards", "stacked", "divided"):
        del RUN[key][:]
    got = {}
    with tf_eager.feeding(G.feed(parts, ds, False, inputs)):
        got["in/src_tokens"] = enc.input_sequence.input_factors[0].numpy()
        got["in/src_ids"] = enc.input_sequence.inputs.numpy()
        got["in/tgt_tokens"] = dec.train_tokens.numpy()
        got["in/tgt_ids"] = dec.train_inputs.numpy()                          # time-major [T, B]
        got["out/loss"] = np.asarray(objective.loss.numpy(), np.float64)
        if mode.get("ce_smoothing", 0.0) > 0.0:
            got["out/cost"] = np.asarray(dec.cost.numpy(), np.float64)
        got["out/name"] = np.asarray(objective.name)
    samples = len(RUN["samples"])
    assert samples == mode["sample_size"] and not RUN["draws"] and (RUN["replay"] is None or not RUN["replay"])
    tmax = cfg["max_output_len"]
    symbols = np.zeros((samples, tmax, cfg["batch"]), np.int32)               # <pad> behind a loop's end
    draws = np.zeros((samples, tmax, cfg["batch"]), np.int32)
    steps = []
    for s, (sym, drawn) in enumerate(RUN["samples"]):
        assert sym.shape == drawn.shape and 1 <= sym.shape[0] <= tmax
        steps.append(sym.shape[0])
        symbols[s, :sym.shape[0]], draws[s, :sym.shape[0]] = sym, drawn
    got["out/symbols"], got["out/draws"], got["out/steps"] = symbols, draws, np.asarray(steps, np.int32)
    got["out/rewards"] = np.stack(RUN["rewards"]).astype(np.float32)
    stacked = [a for a in RUN["stacked"] if a.shape == (samples, cfg["batch"]) and a.dtype == np.float32]
    assert len(stacked) >= 2 and np.array_equal(stacked[-2], got["out/rewards"])
    got["out/sent_logprobs"] = stacked[-1]
    if mode.get("subtract_baseline"):
        got["out/baseline"] = np.asarray(RUN["divided"][-1], np.float32).reshape(())
        got["out/reward_counter"] = np.asarray(RUN["kept"]["reward_counter"].numpy(), np.float32).reshape(())
        got["out/reward_sum"] = np.asarray(RUN["kept"]["reward_sum"].numpy(), np.float32).reshape(())
    else:
        got["out/baseline"] = np.zeros((), np.float32)
    return got


def interesting(runs, cfg):
    """At least one sample's loop ends before max_output_len and at least one does not; some rewards are not zero."""
    steps = np.concatenate([r["out/steps"] for r in runs])
    rewards = np.concatenate([r["out/rewards"].reshape(-1) for r in runs])
    return bool((steps < cfg["max_output_len"]).any() and (steps == cfg["max_output_len"]).any()
                and (rewards != 0).sum() >= 3 and len(set(rewards.tolist())) >= 3)


def run_mode(case, mode_name=None, seeds=4000):
    mode_name = mode_name or case.split("_", 1)[1]
    cfg, mode = dict(CONFIG), dict(MODES[mode_name])
    ds = G.dataset(G.rnn_series(cfg))
    inputs = G.string_inputs("source", "target")
    runs_wanted = 2 if mode.get("subtract_baseline") else 1
    for seed in range(seeds):
        RUN["kept"].clear()
        runs = [evaluate(cfg, mode, ds, inputs, seed=[seed, r]) for r in range(runs_wanted)]
        if interesting(runs, cfg):
            break
    else:
        raise AssertionError("{}: no seed below {} gives both a loop that ends early and one that does not".format(
            case, seeds))
    assert interesting(runs, cfg)
    out = dict(runs[0])
    for r, run in enumerate(runs[1:], 2):
        out.update({"run{}/{}".format(r, k[4:]): v for k, v in run.items() if k.startswith("out/")})
    out["out/variable_names"] = np.asarray(sorted(RUN["kept"]))
    cfg.update(mode=mode, mode_name=mode_name, draw_seed=seed, reward="gleu", runs=runs_wanted)
    G.save(case, cfg, out)
    print("   seed {} steps {} rewards {} baseline {} loss {}".format(
        seed, [r["out/steps"].tolist() for r in runs], runs[0]["out/rewards"].round(3).tolist(),
        [float(r["out/baseline"]) for r in runs], [float(r["out/loss"]) for r in runs]))
    return cfg, runs


def run_fd(case, per_variable=5, h=5e-3):
    cfg, mode = dict(CONFIG), dict(MODES["mixed"])
    ds = G.dataset(G.rnn_series(cfg))
    inputs = G.string_inputs("source", "target")
    with np.load(os.path.join(G.OUT, "reinforce_mixed.npz")) as z:             # the draws of that case, first run
        seed = json.loads(str(z["cfg"]))["draw_seed"]
    bump = {}

    def factory(name, shape, np_dtype, initializer):
        value = G.variable_factory(name, shape, np_dtype, initializer)
        if name in bump:
            idx, delta = bump[name]
            value = value.copy()
            value.reshape(-1)[idx] += np.asarray(delta, value.dtype)
        return value

    RUN["kept"].clear()
    base = evaluate(cfg, mode, ds, inputs, seed=[seed, 0])
    replay = [base["out/draws"][s, :n] for s, n in enumerate(base["out/steps"])]
    held = [r for r in base["out/rewards"]]

    def again():
        RUN["kept"].clear()                                   # every evaluation is a first run: the same baseline
        return evaluate(cfg, mode, ds, inputs, replay=replay, held=held)
    tf_eager.VARIABLE_FACTORY = factory
    try:
        same = again()
        for key in ("out/symbols", "out/steps", "out/rewards", "out/baseline", "out/sent_logprobs", "out/loss"):
            assert np.array_equal(same[key], base[key]), key
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
                up = again()
                bump[name] = (int(i), -h)
                down = again()
                for side in (up, down):        # the draws are replayed and the rewards held: nothing jumps
                    assert np.array_equal(side["out/symbols"], base["out/symbols"])
                    assert np.array_equal(side["out/baseline"], base["out/baseline"])
                names.append(name)
                index.append(int(i))
                value.append((float(up["out/loss"]) - float(down["out/loss"])) / (2.0 * h))
        bump.clear()
        out = again()                                 # leave the unperturbed variables in the store for save()
        out["fd/names"] = np.asarray(names)
        out["fd/index"] = np.asarray(index, np.int64)
        out["fd/value"] = np.asarray(value, np.float64)
        out["fd/h"] = np.asarray(h)
        out["out/variable_names"] = np.asarray(sorted(RUN["kept"]))
    finally:
        tf_eager.VARIABLE_FACTORY = G.variable_factory
    cfg.update(mode=mode, mode_name="mixed", draw_seed=seed, reward="gleu", runs=1)
    G.save(case, cfg, out)


# ---- the rewards ---------------------------------------------------------------------------------------------------------------
def score_inputs():
    """name -> (references [T_ref, B], hypotheses [T_hyp, B]), int64 as the decoder hands them over; ids below 12, the
    size of the model's target vocabulary (4 special symbols and 8 words)."""
    cases = collections.OrderedDict()
    rng = np.random.default_rng(21)
    for bsz in (5, 67):
        for t_ref, t_hyp in ((1, 3), (7, 9), (70, 130)):
            # vocabularies of 3 to 8 words (<pad> and </s> among them): n-grams repeat
            width = rng.integers(3, 9, size=bsz)
            ref = (rng.integers(0, 1 << 30, (t_ref, bsz)) % width).astype(np.int64)
            hyp = (rng.integers(0, 1 << 30, (t_hyp, bsz)) % width).astype(np.int64)
            if t_ref == 70:                       # long sentences: few cuts, or every sentence ends at once
                for arr in (ref, hyp):
                    cut = (arr == END) | (arr == PAD)
                    arr[cut] = np.where(rng.random(int(cut.sum())) < 0.97, 1, arr[cut])
            cases["random_b{}_r{}_h{}".format(bsz, t_ref, t_hyp)] = (ref, hyp)
    columns = [
        ([4, 5, 4, 5, 6, 3], [END, 4, 5, 4, 5, 6]),           # an empty hypothesis
        ([END, 4, 5, 4, 5, 6], [4, 5, 4, 5, 6, 3]),           # an empty reference
        ([END, 4, 5, 4, 5, 6], [PAD, 4, 5, 4, 5, 6]),         # both empty: the empty word matches itself
        ([4, 5, 6, PAD, 7, END], [4, 5, PAD, 6, END, 6]),     # cut by <pad> before </s>
        ([4, 5, 4, 5, 6, 3], [4, 5, 4, END, 5, 6]),           # a hypothesis shorter than 4 words: no 4-gram
        ([4, 5, 4, 5, 6, 3], [5, END, 0, 0, 0, 0]),           # ... of one word
        ([4, 5, 4, 5, 4, 5], [4, 5, 4, 7, 7, END]),           # a repeated hypothesis n-gram, several reference windows
        ([4, 4, 4, 4, 4, 4], [4, 4, END, 0, 0, 0]),           # ... more true positives than hypothesis n-grams
        ([4, 5, 4, 5, 6, 3], [7, 8, 7, 8, 9, 9]),             # nothing in common: the smoothing runs over four orders
        ([4, 5, 6, 7, END, 0], [4, 5, 9, 9, END, 0]),         # ... over the last two
        ([4, 5, 4, 5, 6, 3], [4, 5, 4, 5, 6, 3]),             # equal, no cut
        ([4, 5, 4, 5, END, 0], [4, 5, 4, 5, END, 0]),         # equal, with an end token
        ([4, 5, 6, END, 0, 0], [4, 5, 6, 7, 8, 9]),           # a hypothesis longer than the reference
    ]
    cases["hand_made"] = (np.asarray([c[0] for c in columns], np.int64).T.copy(),
                          np.asarray([c[1] for c in columns], np.int64).T.copy())
    return cases


def run_scores(case):
    cfg = dict(CONFIG)
    ds = G.dataset(G.rnn_series(cfg))
    inputs = G.string_inputs("source", "target")
    out = {}
    for kind in evaluators():
        RUN["kept"].clear()
        evaluate(cfg, dict(sample_size=1), ds, inputs, seed=0, reward=kind)
        score = RUN["score"]                                  # the reference's closure over THIS evaluator
        assert score.__name__ == "_score_with_reward_function"
        for name, (ref, hyp) in score_inputs().items():
            out[name + "/ref"], out[name + "/hyp"] = ref.astype(np.int32), hyp.astype(np.int32)
            got = score(ref, hyp)
            assert got.dtype == np.float32 and got.shape == (ref.shape[1],)
            out[name + "/" + kind] = got
    out["vocabulary"] = np.asarray(G.make_vocab(cfg["tgt_vocab"]).index_to_word)
    os.makedirs(G.OUT, exist_ok=True)
    path = os.path.join(G.OUT, case + ".npz")
    np.savez_compressed(path, **out)
    print("{:28s} {:4d} arrays {:8d} bytes".format(case, len(out), os.path.getsize(path)))


# ---- the reference's configuration and constructors -----------------------------------------------------------------------------
SIGNATURES = os.path.join(HERE, "reinforce_signatures.json")
BUNDLE = os.path.join(HERE, "reference_tests_rl.tar.gz")
CLASSES = [("trainers/rl_trainer.py", "ReinforceObjective"), ("evaluators/gleu.py", "GLEUEvaluator"),
           ("evaluators/bleu.py", "BLEUEvaluator")]


def signatures():
    sys.path.insert(0, os.path.join(G.REPO))
    from tests.test_reference_signatures import read_reference_parameters
    return {path: {name: read_reference_parameters(path, name)} for path, name in CLASSES}


def write_bundle():
    """tests/rl.ini byte for byte (every data file it names is in reference_tests.tar.gz already) and the constructors'
    parameters, as a JSON file beside it and inside the archive."""
    text = json.dumps(signatures(), indent=1, sort_keys=True) + "\n"
    with open(SIGNATURES, "w", encoding="utf-8") as handle:
        handle.write(text)
    with open(os.path.join(G.REFERENCE, "tests", "rl.ini"), "rb") as handle:
        ini = handle.read()
    raw = io.BytesIO()
    with tarfile.open(fileobj=raw, mode="w", format=tarfile.GNU_FORMAT) as tar:
        for rel, data in (("tests/rl.ini", ini), ("reinforce_signatures.json", text.encode())):
            info = tarfile.TarInfo(rel)
            info.size, info.mode, info.mtime = len(data), 0o644, 0
            tar.addfile(info, io.BytesIO(data))
    with open(BUNDLE, "wb") as handle:
        with gzip.GzipFile(fileobj=handle, mode="wb", mtime=0, filename="") as gz:
            gz.write(raw.getvalue())
    print(BUNDLE, os.path.getsize(BUNDLE))


CASES = collections.OrderedDict([
    ("scores", run_scores),
    ("reinforce_bandit", run_mode),
    ("reinforce_mrt", run_mode),
    ("reinforce_google", run_mode),
    ("reinforce_mixed", run_mode),
    ("fd_gradients_reinforce", run_fd),
])


if __name__ == "__main__":
    for name_ in (sys.argv[1:] or list(CASES)):
        CASES[name_](name_)
    if not sys.argv[1:]:
        write_bundle()
