"""The reward kernels of self-critical training (csrc/nm_reward.hip, include/nmhip_reward.h) on the MI355X against the
NumPy functions of trainers/self_critical_objective.py and against what the reference's own functions returned
(tests/golden/self_critical/rewards.npz).

Cases: B = 5 and B = 67 (more sentences than a wavefront has lanes: one wavefront per sentence), (T_ref, T_hyp) = (7, 9),
(1, 3) and (70, 130) -- the two lengths are independent; 130 hypothesis positions are more than the 64 lanes, so a lane
takes several -- over vocabularies of 3 to 8 words, where n-grams repeat and the clipped counts differ from the plain
ones; hand-made columns with the end token at index 0, 1 and 2 (an end token below index n - 1 does not stop the
n-grams), without an end token, a hypothesis equal to its reference and one with nothing in common; a non-contiguous row
stride for both arrays.

Tolerances: the kernel counts in integers and finishes in double, rounding once to float.  GLEU is a quotient of two
integers, correctly rounded on both sides: bit-equal.  BLEU goes through double ``pow`` and ``exp``, whose last double
bit may differ between the device's library and the host's; before the one rounding to float that moves the result
by at most one float32 unit in the last place.  ``nm_reinforce_weights``: the weights are one subtraction, one sign and one
product with 0 or 1 -- bit-equal; the two scalars are one float division each -- 1 ulp."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REWARDS = os.path.join(ROOT, "tests", "golden", "self_critical", "rewards.npz")
HERE = "tests/test_reward_kernels_gpu.py::"
END = 2

pytestmark = pytest.mark.gpu

RANDOM = [(5, 7, 9), (5, 1, 3), (5, 70, 130), (67, 7, 9), (67, 1, 3), (67, 70, 130)]


def ulps(a, b):
    """Distance of two float32 arrays in units in the last place (both non-negative here)."""
    return np.abs(a.astype(np.float32).view(np.int32).astype(np.int64) - b.astype(np.float32).view(np.int32).astype(np.int64))


@pytest.fixture(scope="module")
def golden():
    return np.load(REWARDS)


@pytest.fixture(scope="module")
def host_rewards(golden):
    """The NumPy functions on every case of the fixture, computed once."""
    from neuralmonkey_amd.trainers.self_critical_objective import sentence_bleu, sentence_gleu
    names = sorted({k.split("/")[0] for k in golden.files})
    return {n: (sentence_bleu(golden[n + "/ref"], golden[n + "/hyp"]), sentence_gleu(golden[n + "/ref"], golden[n + "/hyp"]))
            for n in names}


def on_device(kind, ref, hyp, strided=False):
    from neuralmonkey_amd import ops
    dev = "cuda:0"
    if strided:                                  # rows 3 * B + 5 and 2 * B apart, the arrays in the first B columns
        bsz = ref.shape[1]
        wide_r = torch.full((ref.shape[0], 3 * bsz + 5), END, dtype=torch.int32, device=dev)
        wide_h = torch.full((hyp.shape[0], 2 * bsz), END, dtype=torch.int32, device=dev)
        wide_r[:, :bsz] = torch.tensor(ref, device=dev)
        wide_h[:, :bsz] = torch.tensor(hyp, device=dev)
        r, h = wide_r[:, :bsz], wide_h[:, :bsz]
        assert not r.is_contiguous() or bsz == 0
    else:
        r, h = torch.tensor(ref, device=dev), torch.tensor(hyp, device=dev)
    out = ops.sentence_reward(kind, r, h, END)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check(name, golden, host_rewards, strided=False):
    ref, hyp = golden[name + "/ref"], golden[name + "/hyp"]
    bleu, gleu = on_device("bleu", ref, hyp, strided), on_device("gleu", ref, hyp, strided)
    host_bleu, host_gleu = host_rewards[name]
    print(name, "BLEU ulps vs NumPy", int(ulps(bleu, host_bleu).max()), "vs reference", int(ulps(bleu, golden[name + "/bleu"]).max()),
          "nonzero", int((bleu > 0).sum()), "of", bleu.size)
    assert bleu.dtype == np.float32 and gleu.dtype == np.float32
    assert ulps(bleu, host_bleu).max() <= 1 and ulps(bleu, golden[name + "/bleu"]).max() <= 1
    assert np.array_equal((bleu == 0), (host_bleu == 0))                     # an exact zero stays one
    assert gleu.tobytes() == host_gleu.tobytes()
    ok = golden[name + "/gleu_defined"]
    assert np.array_equal(gleu[ok], golden[name + "/gleu"][ok])
    assert np.all(gleu[~ok] == 0.0)                                          # where the reference fails its assertion


@pytest.mark.parametrize("bsz,t_ref,t_hyp", RANDOM)
def test_random_sentences_match_numpy_and_the_reference(golden, host_rewards, bsz, t_ref, t_hyp):
    name = "random_b{}_r{}_h{}".format(bsz, t_ref, t_hyp)
    assert golden[name + "/ref"].shape == (t_ref, bsz) and golden[name + "/hyp"].shape == (t_hyp, bsz)
    assert golden[name + "/ref"].max() < 8 and golden[name + "/hyp"].max() < 8
    check(name, golden, host_rewards)


def test_hand_made_columns(golden, host_rewards):
    hyp, ref = golden["hand_made/hyp"], golden["hand_made/ref"]
    assert [int(np.flatnonzero(hyp[:, b] == END)[0]) for b in range(3)] == [0, 1, 2]
    assert not (hyp[:, 5] == END).any() and np.array_equal(hyp[:, 5], ref[:, 5]) and np.array_equal(hyp[:, 6], ref[:, 6])
    assert not set(hyp[:, 7]) & set(ref[:, 7])
    check("hand_made", golden, host_rewards)
    bleu, gleu = host_rewards["hand_made"]
    assert bleu[0] == 0.0 and gleu[0] > 0.0           # end token at index 0: no unigram, but 2-grams and above
    assert bleu[5] == 1.0 and gleu[5] == 1.0 and bleu[6] == 1.0 and gleu[6] == 1.0
    assert bleu[7] == 0.0 and gleu[7] == 0.0
    assert gleu[8] == np.float32(min(3 / 18, 3 / 18))     # 2 of 6 unigrams and 1 of 5 bigrams survive the clipping


def test_row_strides_of_their_own(golden, host_rewards):
    check("random_b67_r7_h9", golden, host_rewards, strided=True)
    check("hand_made", golden, host_rewards, strided=True)


def test_runs_are_bit_equal_and_lengths_are_bounded(golden):
    from neuralmonkey_amd import _lib, ops
    ref, hyp = golden["random_b67_r70_h130/ref"], golden["random_b67_r70_h130/hyp"]
    first, second = on_device("bleu", ref, hyp), on_device("bleu", ref, hyp)
    assert first.tobytes() == second.tobytes()
    limit = ops.sentence_reward_max_tokens()
    assert limit == 8192
    dev = "cuda:0"
    big = torch.zeros((limit, 1), dtype=torch.int32, device=dev)
    with pytest.raises(_lib.NMHipError, match="above the 8192 the LDS staging holds"):
        ops.sentence_reward("gleu", big, big[:1], END)
    # the longest pair it takes: one sentence, reference of 8191 distinct tokens, hypothesis of one
    long_ref = torch.arange(3, 3 + limit - 1, dtype=torch.int32, device=dev).reshape(-1, 1)
    got = ops.sentence_reward("gleu", long_ref, long_ref[:1].clone(), END)
    torch.cuda.synchronize()
    assert float(got[0]) == np.float32(1.0 / (4 * (limit - 1) - 6))       # recall: 1 of the reference's n-grams


@pytest.mark.parametrize("steps,bsz", [(1, 1), (9, 5), (50, 128), (130, 67)])
def test_reinforce_weights(steps, bsz):
    from neuralmonkey_amd import ops
    rng = np.random.default_rng(steps * 1000 + bsz)
    reward = rng.random(bsz).astype(np.float32)
    baseline = rng.random(bsz).astype(np.float32)
    baseline[::3] = reward[::3]                                       # D = 0
    lengths = rng.integers(1, steps + 1, bsz)
    mask = (np.arange(steps)[:, None] < lengths[None, :]).astype(np.int32)
    weight = 0.5
    dev = "cuda:0"
    w = torch.empty((steps, bsz), dtype=torch.float32, device=dev)
    scale, inv = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)
    ops.reinforce_weights(torch.tensor(reward, device=dev), torch.tensor(baseline, device=dev), torch.tensor(mask, device=dev),
                          weight, w, scale, inv)
    torch.cuda.synchronize()
    want = (-(reward - baseline))[None, :] * mask.astype(np.float32)
    assert w.cpu().numpy().tobytes() == want.tobytes()
    count = np.float32(mask.sum())
    assert ulps(scale.cpu().numpy(), np.float32(weight) / count).max() <= 1
    assert ulps(inv.cpu().numpy(), np.float32(1.0) / count).max() <= 1
    ops.reinforce_weights(torch.tensor(reward, device=dev), torch.tensor(baseline, device=dev),
                          torch.zeros((steps, bsz), dtype=torch.int32, device=dev), weight, w, scale, inv)
    torch.cuda.synchronize()
    assert float(scale[0]) == 0.0 and float(inv[0]) == 0.0 and not w.cpu().numpy().any()


# each entry point of include/nmhip_reward.h -> the test above that calls it (checked in tests/test_self_critical_host.py)
LEDGER = {
    "nm_sentence_reward_max_tokens": HERE + "test_runs_are_bit_equal_and_lengths_are_bounded via ops.sentence_reward_max_tokens",
    "nm_sentence_reward": HERE + "test_runs_are_bit_equal_and_lengths_are_bounded via ops.sentence_reward",
    "nm_reinforce_weights": HERE + "test_reinforce_weights via ops.reinforce_weights",
}
