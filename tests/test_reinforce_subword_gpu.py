"""ReinforceObjective over a vocabulary of BPE pieces on the MI355X: the fixture model of tests/test_reinforce_gpu.py
(tests/golden/reinforce, the mode of tests/rl.ini) with its decoder's 8 words replaced by the pieces
``ab@@ c a@@ bc @@ x@@ y abc`` and its targets by sentences of them.

  * ``ReinforceObjective.rewards`` on the symbols the objective drew itself equals ``score_on_the_host`` on the same
    arrays (GLEU is a quotient of integers, correctly rounded on both sides: EQUAL);
  * with ``score_on_the_host`` patched to raise, a term over replayed samples and a whole training step run -- the
    rewards come from ``nm_eval_joined_sentence_score`` -- and the term's rewards and loss equal those of the host route,
    taken by a second model from which the table is withheld (equal rewards, and from there on the same kernels on the
    same operands: the loss within 1e-6, the bound of test_reinforce_gpu.py::test_an_unknown_callable_takes_the_host_route).
    A tree without the kernel takes the host route here and raises."""
import numpy as np
import pytest

from . import test_reference_exec_gpu as E
from .test_reinforce_gpu import built, forward_term, replaying

pytestmark = pytest.mark.gpu

PIECES = ["ab@@", "c", "a@@", "bc", "@@", "x@@", "y", "abc"]
END, PAD = 2, 0
AB_, C, A_, BC, JOINER, X_, Y, ABC = range(4, 12)
TARGETS = [["ab@@", "c", "y"], ["abc", "y", "abc"], ["a@@", "bc", "x@@", "y"], ["y", "c", "@@", "abc"], ["x@@", "ab@@", "c"]]
# [S = 2, T = 6, B = 5]: the targets' words spelled with other pieces, and sentences that are partly right
SAMPLES = np.asarray([
    [[ABC, Y, END, 0, 0, 0], [A_, BC, Y, AB_, C, END], [AB_, C, X_, Y, END, 0], [Y, C, ABC, END, 0, 0],
     [X_, A_, BC, END, 0, 0]],
    [[AB_, C, C, END, 0, 0], [ABC, ABC, END, 0, 0, 0], [A_, BC, Y, END, 0, 0], [Y, END, 0, 0, 0, 0],
     [X_, AB_, C, Y, END, 0]]], np.int32).transpose(0, 2, 1).copy()


def piece_model(dev, monkeypatch):
    """The fixture's model of the mode of tests/rl.ini over the piece vocabulary (the same sizes: its variables load)."""
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    from neuralmonkey_amd.vocabulary import Vocabulary
    words = E.vocabulary
    monkeypatch.setattr(E, "vocabulary", lambda n: Vocabulary(list(PIECES)) if n == len(PIECES) else words(n))
    _, cfg, _, m, ds, objective, trainer = built(dev, "reinforce_mixed")
    assert cfg["tgt_vocab"] == len(PIECES) and cfg["batch"] == len(TARGETS) and cfg["mode"]["sample_size"] == 2
    assert list(m["dec"].vocabulary.index_to_word) == ["<pad>", "<s>", "</s>", "<unk>"] + PIECES
    series = {"source": ds.get_series("source"), "target": [list(t) for t in TARGETS]}
    pieces = Dataset("pieces", series, BatchingScheme(batch_size=len(TARGETS)))
    assert objective.device_reward() is None and objective.joined_device_reward() == ("gleu", 4)
    return m, pieces, objective, trainer


def test_rewards_equal_the_host_route_on_sampled_symbols(dev, monkeypatch):
    from neuralmonkey_amd.trainers.rl_trainer import score_on_the_host
    m, ds, objective, _ = piece_model(dev, monkeypatch)
    seen = []
    inner = objective.rewards

    def recording(ctx, references, hypotheses, out):
        result = inner(ctx, references, hypotheses, out)
        seen.append((references.cpu().numpy(), hypotheses.cpu().numpy()))
        return result
    objective.rewards = recording
    term = forward_term(m, ds, objective)                         # the objective's own draws
    assert len(seen) == 2 and term["rewards"].shape == (2, 5)
    for s, (ref, hyp) in enumerate(seen):
        assert np.array_equal(hyp, term["symbols"][s])
        want = score_on_the_host(m["dec"].vocabulary, objective.reward_function, ref, hyp.astype(np.int64))
        print("sample", s, "rewards", term["rewards"][s].tolist(), "host", want.tolist())
        assert np.array_equal(term["rewards"][s], want)
    ref = seen[0][0]
    assert ref[:3, 0].tolist() == [AB_, C, Y] and ref[3, 0] == END    # the references are the piece sentences


def test_a_training_step_takes_no_host_route(dev, monkeypatch):
    from neuralmonkey_amd.trainers import rl_trainer
    host = rl_trainer.score_on_the_host

    def refuse(*args, **kwargs):
        raise AssertionError("the rewards of a BPE vocabulary took the host route")
    m, ds, objective, trainer = piece_model(dev, monkeypatch)
    monkeypatch.setattr(rl_trainer, "score_on_the_host", refuse)
    on_device = forward_term(m, ds, objective, samples=SAMPLES)
    assert len(on_device["steps"]) == 2
    assert np.array_equal(on_device["rewards"][0], np.ones(5, np.float32))       # every word respelled: all equal
    assert 0.0 < on_device["rewards"][1].min() < on_device["rewards"][1].max() < 1.0
    replaying(objective, SAMPLES)
    step = m["tfm"].execute(ds, trainer.feedables, [trainer], train=True)[0]      # gradients and an update
    assert list(step.losses) == ["decoder_rl", "L1", "L2"] and np.isfinite(step.losses["decoder_rl"])

    # the host route: a second model, the table withheld
    monkeypatch.setattr(rl_trainer, "score_on_the_host", host)
    m2, ds2, withheld, _ = piece_model(dev, monkeypatch)
    monkeypatch.setattr(rl_trainer, "piece_table", lambda vocabulary: None)
    assert withheld.joined_device_reward() is None
    on_host = forward_term(m2, ds2, withheld, samples=SAMPLES)
    print("loss", float(on_device["loss"]), "through the host", float(on_host["loss"]),
          "rewards", on_device["rewards"].tolist())
    assert np.array_equal(on_device["rewards"], on_host["rewards"])
    assert np.float32(on_device["baseline"]) == np.float32(on_host["baseline"])
    assert abs(float(on_device["loss"]) - float(on_host["loss"])) <= 1e-6
