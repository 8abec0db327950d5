"""The kernels of REINFORCE training (csrc/nm_rl.hip, include/nmhip_rl.h) on the MI355X against what the reference's own
``_score_with_reward_function`` returned with its GLEU and BLEU evaluators (tests/golden/reinforce/scores.npz, see
make_reinforce_golden.py) and against a float64 NumPy restatement of the sample-space arithmetic.

``nm_eval_sentence_score``: B = 5 and B = 67 (one wavefront per sentence, more sentences than a workgroup's lanes),
(T_ref, T_hyp) = (1, 3) (no 2-gram on the reference's side), (7, 9) and (70, 130) (a lane takes several reference
positions and walks more hypothesis positions than a wavefront has lanes), over vocabularies of 3 to 8 words where
n-grams repeat; hand-made columns: an empty hypothesis, an empty reference, both empty, a cut by <pad> before </s>,
hypotheses shorter than 4 words, a repeated hypothesis n-gram that matches several reference windows (true positives
are not clipped), nothing in common (BLEU's smoothing chain), equal sequences; contiguous arrays and row strides of
their own.  The kernel counts in integers and finishes in double, rounding once to float: GLEU is a quotient of two
integers, correctly rounded on both sides -- EQUAL; BLEU goes through double ``log`` and ``exp``, whose last double
bit may differ between the device's library and the host's, which before the one rounding to float moves the result
by at most one float32 unit in the last place.

``nm_reinforce_sample_weights``: S in {1, 3}, B in {1, 5, 67}, loop lengths that differ per sample (rows behind a loop's
end carry weight 0), both flags, two successive calls (the baseline's state).  The kernel computes in double from the
float32 inputs and the float32 baseline and rounds every output once; the restatement does the same in NumPy float64,
so a weight differs by the rounding of the device's double ``exp`` at most: 4 float32 epsilons relative, as the bound
says; the counter is a sum of small integers in float32 -- exact; the running sum adds the rewards up in float32 in the order of
``float32_sum`` below and the baseline is one correctly rounded float32 division, restated operation for operation -- equal;
the loss is a double sum rounded once: 4 float32 epsilons of the sum of its terms' magnitudes."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORES = os.path.join(ROOT, "tests", "golden", "reinforce", "scores.npz")
HERE = "tests/test_rl_kernels_gpu.py::"
END, PAD = 2, 0
EPS32 = float(np.finfo(np.float32).eps)

pytestmark = pytest.mark.gpu

RANDOM = [(5, 1, 3), (5, 7, 9), (5, 70, 130), (67, 1, 3), (67, 7, 9), (67, 70, 130)]


def ulps(a, b):
    """Distance of two float32 arrays in units in the last place (both non-negative here)."""
    return np.abs(a.astype(np.float32).view(np.int32).astype(np.int64) - b.astype(np.float32).view(np.int32).astype(np.int64))


@pytest.fixture(scope="module")
def golden():
    return np.load(SCORES)


def on_device(kind, ref, hyp, strided=False, order=4):
    from neuralmonkey_amd import ops
    dev = "cuda:0"
    if strided:                                  # rows 3 * B + 5 and 2 * B apart, the arrays in the first B columns
        bsz = ref.shape[1]
        wide_r = torch.full((ref.shape[0], 3 * bsz + 5), 4, dtype=torch.int32, device=dev)
        wide_h = torch.full((hyp.shape[0], 2 * bsz), 4, dtype=torch.int32, device=dev)
        wide_r[:, :bsz] = torch.tensor(ref, device=dev)
        wide_h[:, :bsz] = torch.tensor(hyp, device=dev)
        r, h = wide_r[:, :bsz], wide_h[:, :bsz]
        assert (ref.shape[0] == 1 or not r.is_contiguous()) and not h.is_contiguous()    # (one row is contiguous)
    else:
        r, h = torch.tensor(ref, device=dev), torch.tensor(hyp, device=dev)
    out = ops.eval_sentence_score(kind, order, r, h, END, PAD)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check(name, golden):
    ref, hyp = golden[name + "/ref"], golden[name + "/hyp"]
    for strided in (False, True):
        gleu, bleu = on_device("gleu", ref, hyp, strided), on_device("bleu", ref, hyp, strided)
        print(name, "strided" if strided else "contiguous", "BLEU ulps", int(ulps(bleu, golden[name + "/bleu"]).max()),
              "GLEU ulps", int(ulps(gleu, golden[name + "/gleu"]).max()), "nonzero", int((gleu > 0).sum()), "of", gleu.size)
        assert bleu.dtype == np.float32 and gleu.dtype == np.float32
        assert np.array_equal(gleu, golden[name + "/gleu"])
        assert ulps(bleu, golden[name + "/bleu"]).max() <= 1


@pytest.mark.parametrize("bsz,t_ref,t_hyp", RANDOM)
def test_random_sentences_match_the_reference(golden, bsz, t_ref, t_hyp):
    name = "random_b{}_r{}_h{}".format(bsz, t_ref, t_hyp)
    assert golden[name + "/ref"].shape == (t_ref, bsz) and golden[name + "/hyp"].shape == (t_hyp, bsz)
    check(name, golden)


def test_hand_made_columns(golden):
    check("hand_made", golden)
    gleu, bleu = golden["hand_made/gleu"], golden["hand_made/bleu"]
    assert gleu[0] == 0.0 and gleu[1] == 0.0 and gleu[2] == 1.0          # the empty word equals the empty word only
    assert gleu[7] == np.float32(min(11 / 3, 11 / 18))                    # 6 + 5 reference windows for 2 + 1 of the hypothesis
    assert gleu[8] == 0.0 and 0.0 < bleu[8] < 5.0                         # nothing in common: smoothed, not zero
    assert gleu[10] == 1.0 and gleu[11] == 1.0 and ulps(bleu[10:12], np.float32([100.0, 100.0])).max() <= 1


def test_orders_below_four_runs_are_bit_equal_and_lengths_are_bounded(golden):
    from neuralmonkey_amd import _lib, ops
    from neuralmonkey_amd.evaluators.bleu import BLEUEvaluator
    from neuralmonkey_amd.evaluators.gleu import GLEUEvaluator
    from neuralmonkey_amd.trainers.rl_trainer import score_on_the_host
    ref, hyp = golden["random_b67_r70_h130/ref"], golden["random_b67_r70_h130/hyp"]
    first, second = on_device("bleu", ref, hyp), on_device("bleu", ref, hyp)
    assert first.tobytes() == second.tobytes()

    class Words:
        index_to_word = [str(w) for w in golden["vocabulary"]]
    ref, hyp = golden["random_b67_r7_h9/ref"], golden["random_b67_r7_h9/hyp"]
    for order in (1, 2, 3):                              # the host evaluators are the reference for the orders below 4
        assert np.array_equal(on_device("gleu", ref, hyp, order=order),
                              score_on_the_host(Words, GLEUEvaluator(n=order), ref, hyp))
        assert ulps(on_device("bleu", ref, hyp, order=order),
                    score_on_the_host(Words, BLEUEvaluator(n=order), ref, hyp)).max() <= 1
    limit = ops.eval_sentence_score_max_tokens()
    assert limit == 8192
    dev = "cuda:0"
    big = torch.full((limit, 1), 5, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.NMHipError, match="above the 8192 the LDS staging holds"):
        ops.eval_sentence_score("gleu", 4, big, big[:1], END, PAD)
    # the longest pair it takes: one sentence, reference of 8191 distinct tokens, hypothesis of its first one
    long_ref = torch.arange(3, 3 + limit - 1, dtype=torch.int32, device=dev).reshape(-1, 1)
    got = ops.eval_sentence_score("gleu", 4, long_ref, long_ref[:1].clone(), END, PAD)
    torch.cuda.synchronize()
    assert float(got[0]) == np.float32(1.0 / (4 * (limit - 1) - 6))       # recall: 1 of the reference's n-grams


def float32_sum(a):
    """The kernel's order: eight interleaved float32 partial sums combined pairwise, then the tail; fewer than eight in
    order.  (NumPy's own float32 sum takes this order up to 128 numbers.)"""
    f, n = np.float32, len(a)
    if n < 8:
        total = f(0.0)
        for x in a:
            total = f(total + x)
        return total
    r, i = [a[j] for j in range(8)], 8
    while i < n - n % 8:
        r = [f(r[j] + a[i + j]) for j in range(8)]
        i += 8
    total = f(f(f(r[0] + r[1]) + f(r[2] + r[3])) + f(f(r[4] + r[5]) + f(r[6] + r[7])))
    for x in a[i:]:
        total = f(total + x)
    if n <= 128:
        assert total == a.sum()
    return total


def restated(rewards, logprobs, steps, tmax, counter, total, subtract, normalize, alpha):
    """rl_trainer.py:149-185 in float64 from the float32 inputs; the baseline's state in float32 as it is kept."""
    samples, bsz = rewards.shape
    base = np.float32(0.0)
    if subtract:
        counter = np.float32(counter + np.float32(samples * bsz))
        total = np.float32(total + float32_sum(rewards.reshape(-1)))
        base = np.float32(total / max(counter, np.float32(1.0)))
    a = -(rewards.astype(np.float64) - np.float64(base))
    lp = logprobs.astype(np.float64)
    if normalize:
        x = np.float64(np.float32(alpha)) * lp
        p = np.exp(x - x.max(0))
        p /= p.sum(0)
        expected = (a * p).sum(0)
        loss = expected.sum() / bsz
        dlp = np.float64(np.float32(alpha)) * p * (a - expected) / bsz
        magnitude = np.abs(a * p).sum() / bsz
    else:
        loss = (a * lp).sum() / bsz
        dlp = a / bsz
        magnitude = np.abs(a * lp).sum() / bsz
    weights = np.where(np.arange(tmax)[None, :, None] < np.asarray(steps)[:, None, None], -dlp[:, None, :], 0.0)
    return weights, loss, magnitude, base, counter, total


@pytest.mark.parametrize("subtract,normalize", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("samples,bsz", [(1, 1), (1, 5), (3, 5), (3, 67), (1, 67), (3, 1)])
def test_reinforce_sample_weights(samples, bsz, subtract, normalize):
    from neuralmonkey_amd import ops
    rng = np.random.default_rng(samples * 1000 + bsz * 4 + subtract * 2 + normalize)
    dev, tmax, alpha, weight = "cuda:0", 9, 0.7, 0.5
    steps = [int(n) for n in rng.integers(1, tmax + 1, samples)]
    steps[0] = tmax if samples == 1 else 3                               # (3 < tmax: rows behind the loop's end)
    assert samples == 1 or len(set(steps)) > 1 or steps[0] < tmax
    counter = torch.zeros(1, dtype=torch.float32, device=dev)
    total = torch.zeros(1, dtype=torch.float32, device=dev)
    host_counter, host_total = np.float32(0.0), np.float32(0.0)
    for call in range(2):                                                # the second call starts from the first's state
        rewards = rng.random((samples, bsz)).astype(np.float32)
        logprobs = (-8.0 * rng.random((samples, bsz))).astype(np.float32)
        outs = []
        for _ in range(2):                                               # two runs from one state: bit-equal
            c, t = counter.clone(), total.clone()
            w = torch.full((samples, tmax, bsz), 7.0, dtype=torch.float32, device=dev)
            scale, loss, base = (torch.full((1,), 7.0, dtype=torch.float32, device=dev) for _ in range(3))
            ops.reinforce_sample_weights(torch.tensor(rewards, device=dev), torch.tensor(logprobs, device=dev), steps, w,
                                         scale, loss, base, weight=weight, subtract_baseline=subtract, normalize=normalize,
                                         alpha=alpha, reward_counter=c if subtract else None,
                                         reward_sum=t if subtract else None)
            torch.cuda.synchronize()
            outs.append([x.cpu().numpy() for x in (w, scale, loss, base, c, t)])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(*outs))
        w, scale, loss, base, c, t = outs[0]
        counter, total = torch.tensor(c, device=dev), torch.tensor(t, device=dev)
        want_w, want_loss, magnitude, want_base, host_counter, host_total = restated(
            rewards, logprobs, steps, tmax, host_counter, host_total, subtract, normalize, alpha)
        err = np.abs(w.astype(np.float64) - want_w)
        print(call, "weights: worst relative error", float((err / np.maximum(np.abs(want_w), 1e-300)).max()) / EPS32, "eps;",
              "loss", float(loss[0]), "restated", want_loss, "baseline", float(base[0]), float(want_base))
        assert np.all(err <= 4 * EPS32 * np.abs(want_w))
        behind = np.broadcast_to(np.arange(tmax)[None, :, None] >= np.asarray(steps)[:, None, None], w.shape)
        assert np.all(w[behind] == 0.0) and (samples == 1 or behind.any())
        assert float(scale[0]) == np.float32(weight)
        assert abs(float(loss[0]) - want_loss) <= 4 * EPS32 * magnitude
        if subtract:
            assert float(c[0]) == float(host_counter) == (call + 1) * samples * bsz        # exact
            assert float(t[0]) == float(host_total) and float(base[0]) == float(want_base)
        else:
            assert float(base[0]) == 0.0 and float(c[0]) == 0.0 and float(t[0]) == 0.0     # the state is not touched


def test_sample_weights_without_sentence_logprobs_and_the_sample_limit():
    from neuralmonkey_amd import _lib, ops
    dev = "cuda:0"
    limit = ops.reinforce_sample_weights_max_samples()
    assert limit == 64
    rewards = torch.rand((limit, 5), device=dev)
    w = torch.empty((limit, 4, 5), device=dev)
    scale, base = torch.empty(1, device=dev), torch.empty(1, device=dev)
    ops.reinforce_sample_weights(rewards, None, [1 + s % 4 for s in range(limit)], w, scale, None, base, weight=2.0)
    torch.cuda.synchronize()
    want = np.where(np.arange(4)[None, :, None] < np.asarray([1 + s % 4 for s in range(limit)])[:, None, None],
                    (rewards.cpu().numpy().astype(np.float64) / 5)[:, None, :], 0.0).astype(np.float32)
    assert np.array_equal(w.cpu().numpy(), want) and float(scale[0]) == 2.0 and float(base[0]) == 0.0
    with pytest.raises(_lib.NMHipError, match=r"bad sizes S 65 \(1..64\)"):
        ops.reinforce_sample_weights(torch.rand((65, 5), device=dev), None, [1] * 65, torch.empty((65, 4, 5), device=dev),
                                     scale, None, base)
    with pytest.raises(_lib.NMHipError, match="loop length 5 of sample 1 outside 1..4"):
        ops.reinforce_sample_weights(rewards[:2].contiguous(), None, [1, 5], w[:2].contiguous(), scale, None, base)


# each entry point of include/nmhip_rl.h -> the test above that calls it (checked in tests/test_reinforce_host.py)
LEDGER = {
    "nm_eval_sentence_score_max_tokens": HERE + "test_orders_below_four_runs_are_bit_equal_and_lengths_are_bounded via "
                                                "ops.eval_sentence_score_max_tokens",
    "nm_eval_sentence_score": HERE + "test_orders_below_four_runs_are_bit_equal_and_lengths_are_bounded via "
                                     "ops.eval_sentence_score",
    "nm_reinforce_sample_weights_max_samples": HERE + "test_sample_weights_without_sentence_logprobs_and_the_sample_limit via "
                                                      "ops.reinforce_sample_weights_max_samples",
    "nm_reinforce_sample_weights": HERE + "test_reinforce_sample_weights via ops.reinforce_sample_weights",
}
