"""ReinforceObjective on the MI355X against what the reference's own Python computed (tests/golden/reinforce, see
make_reinforce_golden.py) and against the float64 restatement of tests/reinforce_ref.py.

  * every fixture case (bandit, MRT, Google, mixed = tests/rl.ini) on the fixture's model, its variables loaded by name,
    the reference's recorded draws replayed through ``samples=``: the rewards, the baseline and every sample's loop
    length are EQUAL, the sentence log-probabilities and the loss agree within 1e-4 relative; where there is a baseline
    the second consecutive run (the carried counter and sum) matches too;
  * the mode of tests/rl.ini: the gradient meets the central differences of the reference's loss within
    6e-3 + 2e-2 |fd| (the bound of tests/test_labeler_host.py) at every recorded coordinate of every variable;
  * every mode: the gradient against float64 autograd of the restatement by the unit method of
    tests/test_self_critical_gpu.py::test_gradients_against_float64_autograd: unit = the restatement evaluated in
    float32 against itself in float64 (never below one float32 epsilon of the largest magnitude), 16 units, capped by
    1e-4 relative on the loss and 1e-3 of the largest magnitude on a gradient; ``attention/attn_bias`` as there;
  * a callable the objective does not know (the same GLEU behind another name) takes the host route, is called once per
    sentence and sample, earns the kernel's rewards exactly (GLEU is a quotient of integers, correctly rounded on both
    sides) and gives its loss within 1e-6 (the same kernels on the same operands from there on);
  * without ``samples=``: one seed draws the same symbols twice, another seed draws others, and every draw is the
    argmax of the returned logits plus the restated Gumbel noise of the loop's salts (tests/test_sampling_gpu.py);
  * the reference's tests/rl.ini from the committed archives, verbatim: three optimizer steps, finite losses under the
    reference's names, the counter of the baseline, the runner decodes, a checkpoint carries the baseline's state."""
import functools
import os
import tarfile

import numpy as np
import pytest
import torch

from . import reinforce_ref as R
from .test_reference_exec_gpu import build_rnn, dataset_of, load_variables
from .test_reference_inis import BUNDLE, load_verbatim
from .test_reinforce_host import BUNDLE as RL_BUNDLE, MODE_CASES, load_fixture
from .test_sampling_gpu import _check_draws
from .test_self_critical_gpu import EPS32, MULTIPLE, ZERO_BY_SYMMETRY, gradients

pytestmark = pytest.mark.gpu


def built(dev, case, reward=None, seed=1, **mode_overrides):
    """The fixture's model with a ReinforceObjective in the fixture's mode.  The session is initialised AFTER the
    objective exists: its store then holds the baseline's two scalars."""
    from neuralmonkey_amd.evaluators.gleu import GLEUEvaluator
    from neuralmonkey_amd.tf_manager import TensorFlowManager
    from neuralmonkey_amd.trainers import GenericTrainer
    from neuralmonkey_amd.trainers.rl_trainer import ReinforceObjective
    z, cfg, params = load_fixture(case)
    m = build_rnn(dev, cfg)
    objective = ReinforceObjective(m["dec"], reward or GLEUEvaluator(), **dict(cfg["mode"], **mode_overrides))
    m["tfm"] = TensorFlowManager(num_sessions=1, num_threads=1, device=str(dev), seed=seed)
    m["tfm"].initialize_sessions()
    m["store"] = m["tfm"].sessions[0].store
    kept = [str(n) for n in z["out/variable_names"]]
    assert kept == (["reward_counter", "reward_sum"] if cfg["mode"].get("subtract_baseline") else [])
    assert sorted(set(m["store"].names()) - set(params)) == kept          # the reference's names for them
    assert load_variables(m["store"], dict(params, **{n: np.zeros((), np.float32) for n in kept})) == []
    trainer = GenericTrainer([objective], l2_weight=0.0, clip_norm=None)
    return z, cfg, params, m, dataset_of(z, cfg), objective, trainer


def forward_term(m, ds, objective, samples=None):
    """The objective's term without a training step: what it drew, what it earned, its loss."""
    from neuralmonkey_amd.runtime import RunContext
    fd = {}
    for part in m["feedables"]:
        fd.update(part.feed_dict(ds, train=False))
    ctx = RunContext(m["tfm"].sessions[0], fd)
    for part in m["feedables"]:
        part.stage_inputs(ctx)
    if samples is not None:
        samples = torch.tensor(np.ascontiguousarray(samples, np.int32))
    term = objective.forward_backward(ctx, 1.0, want_grad=False, samples=samples)
    torch.cuda.synchronize()
    host = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else v
    return {k: ([host(x) for x in v] if isinstance(v, list) else host(v)) for k, v in term.items()}


def replaying(objective, draws):
    """The trainer calls ``forward_backward`` without ``samples``: hand it the recorded draws."""
    samples = torch.tensor(np.ascontiguousarray(draws, np.int32))
    objective.forward_backward = functools.partial(type(objective).forward_backward, objective, samples=samples)


def close(got, want, rel):
    return np.all(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) <= rel * np.abs(np.asarray(want, np.float64)))


@pytest.mark.parametrize("case", MODE_CASES)
def test_engine_equals_the_reference(dev, case):
    z, cfg, _, m, ds, objective, _ = built(dev, case)
    assert objective.name == str(z["out/name"]) == "decoder_rl" and objective.device_reward() == ("gleu", 4)
    for run in ["out/"] + ["run{}/".format(r) for r in range(2, cfg["runs"] + 1)]:     # consecutive runs, one session
        term = forward_term(m, ds, objective, samples=z[run + "draws"])
        print(case, run, "steps", term["steps"], "baseline", float(term["baseline"]), float(z[run + "baseline"]),
              "loss", float(term["loss"]), float(z[run + "loss"]))
        assert term["steps"] == z[run + "steps"].tolist()
        for s, n in enumerate(term["steps"]):
            assert np.array_equal(term["symbols"][s], z[run + "symbols"][s, :n])
        assert term["rewards"].dtype == np.float32 and np.array_equal(term["rewards"], z[run + "rewards"])
        assert np.float32(term["baseline"]) == z[run + "baseline"]
        assert close(term["sent_logprobs"], z[run + "sent_logprobs"], 1e-4)
        assert close(term["loss"], z[run + "loss"], 1e-4)
        if cfg["mode"].get("subtract_baseline"):
            torch.cuda.synchronize()
            assert float(m["store"]["reward_counter"]) == float(z[run + "reward_counter"])
            assert close(float(m["store"]["reward_sum"]), z[run + "reward_sum"], 2 * EPS32)
    steps = np.concatenate([z[k] for k in z.files if k.endswith("/steps")])
    assert (steps < m["dec"].max_output_len).any() and (steps == m["dec"].max_output_len).any()


def test_gradients_against_the_reference_finite_differences(dev):
    z, _, _, m, ds, objective, trainer = built(dev, "fd_gradients_reinforce")
    replaying(objective, z["out/draws"])
    res = m["tfm"].execute(ds, trainer.feedables, [trainer], train=True)[0]
    assert list(res.losses) == ["decoder_rl", "L1", "L2"]
    assert close(res.losses["decoder_rl"], z["out/loss"], 1e-4)
    got, seen = gradients(m), set()
    for name, i, fd in zip([str(n) for n in z["fd/names"]], z["fd/index"], z["fd/value"]):
        g = float(got[name].reshape(-1)[int(i)])
        assert abs(g - fd) <= 6e-3 + 2e-2 * abs(fd), "{}[{}]: engine {:.6f} vs finite difference {:.6f}".format(
            name, i, g, fd)
        seen.add(name)
    assert seen == set(m["store"].trainable_names()) == set(m["store"].names()) - {"reward_counter", "reward_sum"}
    assert not got["reward_counter"].any() and not got["reward_sum"].any()


@pytest.mark.parametrize("case", MODE_CASES)
def test_gradients_against_float64_autograd(dev, case):
    z, cfg, params, m, ds, objective, trainer = built(dev, case)
    replaying(objective, z["out/draws"])
    res = m["tfm"].execute(ds, trainer.feedables, [trainer], train=True)[0]
    got = gradients(m)
    args = (params, z["in/src_ids"], z["in/tgt_ids"], z["out/symbols"], z["out/steps"], z["out/rewards"],
            z["out/baseline"], cfg["mode"])
    loss64, g64, _ = R.loss_and_gradients(*args, dtype=torch.float64)
    loss32, g32, _ = R.loss_and_gradients(*args, dtype=torch.float32)
    unit = max(abs(loss32 - loss64), EPS32 * abs(loss64))
    bound = min(MULTIPLE * unit, 1e-4 * abs(loss64))
    loss = res.losses["decoder_rl"]
    print("loss {:.8f}: error {:.3g} (unit {:.3g}, bound {:.3g})".format(loss, abs(loss - loss64), unit, bound))
    assert abs(loss - loss64) <= bound
    for name in sorted(g64):
        want = g64[name].reshape(got[name].shape)
        mag = float(np.abs(want).max())
        unit = max(float(np.abs(g32[name].reshape(want.shape) - want).max()), EPS32 * mag)
        bound = min(MULTIPLE * unit, 1e-3 * mag)
        if name in ZERO_BY_SYMMETRY:             # float64 leaves its own rounding there: no magnitude to cap by
            assert mag < 1e-15, (name, mag)
            bound = MULTIPLE * unit
        err = float(np.abs(got[name].astype(np.float64) - want).max())
        print("d {}: error {:.3g} (unit {:.3g}, bound {:.3g}, magnitude {:.3g})".format(name, err, unit, bound, mag))
        assert (mag > 0 or name in ZERO_BY_SYMMETRY) and err <= bound, (name, err, bound)


def test_an_unknown_callable_takes_the_host_route(dev):
    from neuralmonkey_amd.evaluators.gleu import GLEUEvaluator
    gleu, calls = GLEUEvaluator(), []

    def gleu_on_the_host(hypotheses, references):
        calls.append((hypotheses, references))
        return gleu(hypotheses, references)
    z, cfg, _, m, ds, known, _ = built(dev, "reinforce_mrt")
    a = forward_term(m, ds, known, samples=z["out/draws"])
    _, _, _, m2, ds2, unknown, _ = built(dev, "reinforce_mrt", reward=gleu_on_the_host)
    assert unknown.device_reward() is None and not calls
    b = forward_term(m2, ds2, unknown, samples=z["out/draws"])
    assert len(calls) == cfg["mode"]["sample_size"] * cfg["batch"] == 15
    hyps, refs = calls[0]
    assert len(hyps) == len(refs) == 1 and all(isinstance(w, str) for w in hyps[0] + refs[0])
    print("loss", float(a["loss"]), "through the host", float(b["loss"]))
    assert np.array_equal(a["rewards"], b["rewards"]) and np.array_equal(b["rewards"], z["out/rewards"])
    assert abs(float(a["loss"]) - float(b["loss"])) <= 1e-6


def test_own_draws_are_reproducible_and_follow_the_logits(dev):
    terms = {}
    for tag, seed in (("a", 1), ("b", 1), ("c", 2)):
        _, _, _, m, ds, objective, _ = built(dev, "reinforce_google", seed=seed)
        terms[tag] = forward_term(m, ds, objective)
    a, b, c = terms["a"], terms["b"], terms["c"]
    assert a["steps"] == b["steps"] and all(np.array_equal(x, y) for x, y in zip(a["symbols"], b["symbols"]))
    assert np.array_equal(a["rewards"], b["rewards"]) and float(a["loss"]) == float(b["loss"])
    assert a["steps"] != c["steps"] or any(not np.array_equal(x, y) for x, y in zip(a["symbols"], c["symbols"]))
    assert a["salts"][0] != a["salts"][1]                                 # every sample's loop draws with its own salts
    for sym, logits, salts in zip(a["symbols"], a["logits"], a["salts"]):
        assert logits.shape[:2] == sym.shape
        # the logits are the device's own, bit for bit; the NOISE is restated on the host (a float32 log of a log), so a
        # near-tie within _check_draws' 1e-4 may still pick the other symbol: the share of test_sampling_gpu.py
        assert _check_draws(sym, logits, salts) >= 0.95


@pytest.fixture(scope="module")
def rl_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("reference_tests_rl")
    for bundle in (BUNDLE, RL_BUNDLE):
        with tarfile.open(bundle) as tar:
            tar.extractall(root)
    return str(root)


def test_rl_ini_trains_decodes_and_checkpoints(dev, rl_root):
    from neuralmonkey_amd.dataset import BatchingScheme
    from neuralmonkey_amd.trainers.rl_trainer import ReinforceObjective
    model = load_verbatim(rl_root, "rl", device=str(dev), seed=1234)
    tfm, trainer = model.tf_manager, model.trainers[0]
    assert isinstance(trainer.objectives[0], ReinforceObjective)
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    store = tfm.sessions[0].store
    step0, seen = tfm.sessions[0].global_step, 0
    for batch in model.train_dataset.batches(BatchingScheme(batch_size=model.batch_size)):
        res = tfm.execute(batch, feedables, model.trainers, train=True)[0]
        assert len(batch) == 16 and list(res.losses) == ["decoder_rl", "L1", "L2"]
        assert all(np.isfinite(v) for v in res.losses.values()), res.losses
        seen += 1
        if seen == 3:
            break
    assert seen == 3 and tfm.sessions[0].global_step == step0 + 3
    torch.cuda.synchronize()
    counter, total = float(store["reward_counter"]), float(store["reward_sum"])
    assert counter == 3 * 16 * 2 and 0.0 <= total <= counter
    val = next(model.val_dataset.batches(BatchingScheme(batch_size=model.batch_size)))
    out = tfm.execute(val, feedables, model.runners, compute_losses=True)
    assert len(out[0].outputs["target"]) == len(val)
    path = os.path.join(rl_root, "baseline_checkpoint")
    tfm.save(path)
    store["reward_counter"].fill_(0.0)
    store["reward_sum"].fill_(-1.0)
    tfm.restore(path)
    torch.cuda.synchronize()
    assert float(store["reward_counter"]) == counter and float(store["reward_sum"]) == total
