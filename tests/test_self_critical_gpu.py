"""SelfCriticalObjective on the MI355X against what the reference's own Python computed
(tests/golden/self_critical, see make_self_critical_golden.py) and against the float64 restatement of
tests/self_critical_ref.py.

  * the fixture's model (a GRU decoder of 6 over a bidirectional GRU encoder of 5: the taped path), its variables loaded
    by name and its strings fed: tf.argmax of the teacher-forced and of the runtime logits, the runtime mask and
    D = reward(runtime) - reward(train) are EQUAL, the loss agrees within 1e-4 relative;
  * one training step: the gradient meets the central differences of the reference's loss within 6e-3 + 2e-2 |fd| (the
    bound of tests/test_labeler_host.py) at every recorded coordinate of every variable;
  * ... and the float64 autograd gradient of the restatement by the unit method of
    tests/test_labeler_gpu.py::test_head_gradients_against_float64_autograd: unit = the restatement evaluated in float32
    against itself in float64 (never below one float32 epsilon of the largest magnitude), 16 units, capped by 1e-4
    relative on the loss and 1e-3 of the largest magnitude on a gradient.  The gradient of ``attention/attn_bias``
    vanishes identically (softmax is shift-invariant): float64 autograd returns 1e-18 of its own rounding, the cap by a
    magnitude means nothing there and the bound is the 16 units alone -- measured: error 3.5e-10, unit 2.3e-10;
  * beside a CostObjective over the same decoder: the cost term's loss is the loss of the cost term alone (the same
    kernels on the same operands: equal), the gradient is the weighted sum of the two terms taken alone.  The three are
    float32 sums of at most a few hundred products each, taken in different orders: 1e-5 of the largest magnitude
    (84 float32 epsilons) covers that and nothing else.  Also with a decoder of 8 (seeded variables, a scripted reward), whose
    cost term runs on the hand-scheduled path that OVERWRITES its slices of the flat gradient while the self-critical
    tape adds to them;
  * a reward function the objective does not know (the same BLEU behind another name) takes the host path and gives the
    loss the kernel gives: the device's BLEU is within 1 float32 ulp of the host's (<= 6e-8 on a reward <= 1, 1.2e-7 on
    D), and the loss is a mean of D * nll with nll <= log(12) + the logits' range < 8: 1e-6 absolute;
  * the reference's tests/self-critical.ini from the committed archives, verbatim: three optimizer steps, finite losses
    under the reference's names, the runner decodes."""
import tarfile

import numpy as np
import pytest
import torch

from . import self_critical_ref as R
from .test_reference_exec_gpu import build_rnn, dataset_of, load_variables
from .test_reference_inis import BUNDLE, load_verbatim
from .test_self_critical_host import BUNDLE as SC_BUNDLE, load_fixture

pytestmark = pytest.mark.gpu

MULTIPLE = 16.0
EPS32 = float(np.finfo(np.float32).eps)
# attn_bias is added to every energy of a softmax row alike: the loss does not depend on it and its gradient is a sum
# that cancels exactly
ZERO_BY_SYMMETRY = {"attention/attn_bias"}


def built(dev, case="self_critical_gru", **overrides):
    z, cfg, params = load_fixture(case)
    cfg = dict(cfg, **overrides)
    m = build_rnn(dev, cfg)
    if not overrides:
        assert load_variables(m["store"], params) == []
    else:            # another model: seeded values at the scale of the fixture's (its initialisers' are too small to decode
        store = m["store"]                                             # anything but one word)
        rng = np.random.default_rng(5)
        store.load_state_dict({n: ((1.0 if n.endswith("gamma") else 0.0) + rng.normal(0, 0.35, tuple(store[n].shape)))
                               .astype(np.float32) for n in store.names()})
    return z, cfg, params, m, dataset_of(z, cfg)


def trainer_of(m, kinds, reward=None, weights=(None, None)):
    from neuralmonkey_amd.trainers import CostObjective, GenericTrainer
    from neuralmonkey_amd.trainers.self_critical_objective import SelfCriticalObjective, sentence_bleu
    objectives = []
    for kind, weight in zip(kinds, weights):
        objectives.append(CostObjective(m["dec"], weight=weight) if kind == "cost" else
                          SelfCriticalObjective(m["dec"], reward or sentence_bleu, weight=weight))
    return GenericTrainer(objectives, l2_weight=0.0, clip_norm=None), objectives


def gradients(m):
    torch.cuda.synchronize()
    return {n: m["store"].g(n).detach().cpu().numpy().copy() for n in m["store"].names()}


def forward_term(m, ds, objective):
    """The objective's term without a training step: what it decoded, what it earned, its loss."""
    from neuralmonkey_amd.runtime import RunContext
    fd = {}
    for part in m["feedables"]:
        fd.update(part.feed_dict(ds, train=False))
    ctx = RunContext(m["tfm"].sessions[0], fd)
    for part in m["feedables"]:
        part.stage_inputs(ctx)
    term = objective.result(ctx)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in term.items()}, fd


def test_engine_equals_the_reference(dev):
    z, _, _, m, ds = built(dev)
    _, (objective,) = trainer_of(m, ["critic"])
    assert objective.name == str(z["out/name"]) == "decoder_self_critical"
    term, fd = forward_term(m, ds, objective)
    assert np.array_equal(fd[m["dec"].train_tokens].T, z["in/tgt_ids"])
    assert np.array_equal(term["train_argmax"], z["out/train_argmax"])
    assert np.array_equal(term["runtime_argmax"], z["out/runtime_argmax"])
    assert term["steps"] == z["out/runtime_argmax"].shape[0] < m["dec"].max_output_len      # the loop stopped early
    assert np.array_equal(term["mask"], z["out/runtime_mask"].astype(np.int32))
    diff, want = term["reward"] - term["baseline"], z["out/runtime_reward"] - z["out/train_reward"]
    print("D", diff, "reference", want, "loss", float(term["loss"]), "reference", float(z["out/loss"]))
    assert diff.dtype == np.float32 and np.array_equal(diff, want)
    assert (want != 0).sum() >= 3 and (want > 0).any() and (want < 0).any()
    assert abs(float(term["loss"]) - float(z["out/loss"])) <= 1e-4 * abs(float(z["out/loss"]))


def test_gradients_against_the_reference_finite_differences(dev):
    z, _, _, m, ds = built(dev, "fd_gradients_self_critical")
    trainer, _ = trainer_of(m, ["critic"])
    res = m["tfm"].execute(ds, trainer.feedables, [trainer], train=True)[0]
    assert list(res.losses) == ["decoder_self_critical", "L1", "L2"]
    assert abs(res.losses["decoder_self_critical"] - float(z["out/loss"])) <= 1e-4 * abs(float(z["out/loss"]))
    got, seen = gradients(m), set()
    for name, i, fd in zip([str(n) for n in z["fd/names"]], z["fd/index"], z["fd/value"]):
        g = float(got[name].reshape(-1)[int(i)])
        assert abs(g - fd) <= 6e-3 + 2e-2 * abs(fd), "{}[{}]: engine {:.6f} vs finite difference {:.6f}".format(
            name, i, g, fd)
        seen.add(name)
    assert seen == set(m["store"].names())


def test_gradients_against_float64_autograd(dev):
    z, _, params, m, ds = built(dev)
    trainer, _ = trainer_of(m, ["critic"])
    res = m["tfm"].execute(ds, trainer.feedables, [trainer], train=True)[0]
    got = gradients(m)
    diff = z["out/runtime_reward"].astype(np.float64) - z["out/train_reward"].astype(np.float64)
    loss64, g64, _, _ = R.loss_and_gradients(params, z["in/src_ids"], z["out/runtime_argmax"], diff, torch.float64)
    loss32, g32, _, _ = R.loss_and_gradients(params, z["in/src_ids"], z["out/runtime_argmax"], diff, torch.float32)
    unit = max(abs(loss32 - loss64), EPS32 * abs(loss64))
    bound = min(MULTIPLE * unit, 1e-4 * abs(loss64))
    loss = res.losses["decoder_self_critical"]
    print("loss {:.8f}: error {:.3g} (unit {:.3g}, bound {:.3g})".format(loss, abs(loss - loss64), unit, bound))
    assert abs(loss - loss64) <= bound
    for name in sorted(got):
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


class Scripted:
    """A reward whatever the model decodes: the sentence's index over the batch size on every first call (the runtime
    hypotheses), one half on every second (the train-time ones) -- D takes both signs.  That the gradient is a weighted
    sum does not depend on what the reward means."""

    def __init__(self):
        self.calls = 0

    def __call__(self, references, hypotheses):
        self.calls += 1
        bsz = np.asarray(hypotheses).shape[1]
        return (np.arange(bsz) / bsz if self.calls % 2 else np.full(bsz, 0.5)).astype(np.float32)


@pytest.mark.parametrize("rnn_size", [6, 8])
def test_beside_a_cost_objective_the_gradient_is_the_weighted_sum(dev, rnn_size):
    """rnn_size 6: the fixture's model, both terms on the tape.  rnn_size 8 (fresh variables, seeded): the cost term on
    the hand-scheduled path."""
    overrides = {} if rnn_size == 6 else {"rnn_size": 8}
    grads, losses = {}, {}
    for kinds in (("cost",), ("critic",), ("cost", "critic")):
        _, _, _, m, ds = built(dev, **overrides)
        assert m["dec"].uses_general_path(True) == (rnn_size == 6)
        trainer, _ = trainer_of(m, kinds, reward=None if rnn_size == 6 else Scripted(), weights=(0.5, 0.5))
        losses[kinds] = dict(m["tfm"].execute(ds, trainer.feedables, [trainer], train=True)[0].losses)
        grads[kinds] = gradients(m)
    both = losses[("cost", "critic")]
    assert list(both) == ["decoder - cost", "decoder_self_critical", "L1", "L2"]
    assert both["decoder - cost"] == losses[("cost",)]["decoder - cost"]
    assert both["decoder_self_critical"] == losses[("critic",)]["decoder_self_critical"]
    for name, total in grads[("cost", "critic")].items():
        a, b = grads[("cost",)][name], grads[("critic",)][name]
        mag = max(float(np.abs(a).max()), float(np.abs(b).max()))
        err = float(np.abs(total - (a + b)).max())
        print("{} {}: |cost| {:.3g} |critic| {:.3g} error {:.3g}".format(rnn_size, name, float(np.abs(a).max()),
                                                                        float(np.abs(b).max()), err))
        if name not in ZERO_BY_SYMMETRY:
            assert float(np.abs(a).max()) > 0 and float(np.abs(b).max()) > 0, name
        assert err <= 1e-5 * mag, (name, err, mag)


def test_a_python_reward_function_gives_the_loss_the_kernel_gives(dev):
    from neuralmonkey_amd.trainers.self_critical_objective import sentence_bleu
    calls = []

    def bleu_on_the_host(references, hypotheses):
        calls.append((references.copy(), hypotheses.copy()))
        return sentence_bleu(references, hypotheses)
    z, _, _, m, ds = built(dev)
    _, (known,) = trainer_of(m, ["critic"])
    _, (unknown,) = trainer_of(m, ["critic"], reward=bleu_on_the_host)
    a, _ = forward_term(m, ds, known)
    assert not calls
    b, _ = forward_term(m, ds, unknown)
    assert len(calls) == 2                                        # runtime and train-time hypotheses
    assert np.array_equal(calls[0][0], z["in/tgt_ids"]) and np.array_equal(calls[0][1], z["out/runtime_argmax"])
    assert np.array_equal(calls[1][1], z["out/train_argmax"]) and calls[0][1].dtype == np.int64
    print("loss", float(a["loss"]), "through the host", float(b["loss"]))
    assert abs(float(a["loss"]) - float(b["loss"])) <= 1e-6


@pytest.fixture(scope="module")
def sc_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("reference_tests_self_critical")
    for bundle in (BUNDLE, SC_BUNDLE):
        with tarfile.open(bundle) as tar:
            tar.extractall(root)
    return str(root)


def test_self_critical_ini_trains_and_decodes(dev, sc_root):
    from neuralmonkey_amd.dataset import BatchingScheme
    from neuralmonkey_amd.trainers.self_critical_objective import SelfCriticalObjective
    model = load_verbatim(sc_root, "self-critical", device=str(dev), seed=1234)
    tfm, trainer = model.tf_manager, model.trainers[0]
    assert isinstance(trainer.objectives[1], SelfCriticalObjective)
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    step0, seen = tfm.sessions[0].global_step, 0
    for batch in model.train_dataset.batches(BatchingScheme(batch_size=model.batch_size)):
        res = tfm.execute(batch, feedables, model.trainers, train=True)[0]
        assert list(res.losses) == ["decoder - cost", "decoder_self_critical", "L1", "L2"]
        assert all(np.isfinite(v) for v in res.losses.values()), res.losses
        seen += 1
        if seen == 3:
            break
    assert seen == 3 and tfm.sessions[0].global_step == step0 + 3
    val = next(model.val_dataset.batches(BatchingScheme(batch_size=model.batch_size)))
    out = tfm.execute(val, feedables, model.runners, compute_losses=True)
    assert len(out[0].outputs["target"]) == len(val)
