"""nm_chrf_reward and nm_chrf_pairwise (csrc/nm_chrf.hip) on the MI355X against the Counter restatement of
tests/chrf_ref.py over its twelve-word vocabulary, and their two callers end to end.  Counts are integers and compared
exactly.  Scores lie in [0, 1] and are a double result rounded once to float32, which errs by at most 2^-25 there; the
bound 2^-23 leaves two bits for the order of the double arithmetic."""
import numpy as np
import pytest
import torch

from . import chrf_ref as C
from .test_chrf_host import VARIANTS
from .test_edit_gpu import strided

pytestmark = pytest.mark.gpu

TOLERANCE = 2.0 ** -23


@pytest.mark.parametrize("n,beta,ignored,join", VARIANTS)
@pytest.mark.parametrize("t_hyp,t_ref,bsz,first", C.REWARD_SHAPES)
def test_reward_and_counts_are_the_counter_restatement(dev, t_hyp, t_ref, bsz, first, n, beta, ignored, join):
    from neuralmonkey_amd import ops
    from neuralmonkey_amd.trainers.self_critical_objective import SentenceChrF
    vocab = C.vocabulary()
    table = SentenceChrF(vocab, n, beta, ignored, join).device_table(dev)
    refs, hyps = C.batch(t_hyp, t_ref, bsz, first)
    want, want_counts = C.batch_scores(refs, hyps, vocab.index_to_word, n, beta, ignored or (), join)
    runs = []
    for extra in (3, 3, 0):                                                      # two equal runs; contiguous rows
        counts = torch.full((bsz, 3, 6), -7, dtype=torch.int32, device=dev)
        reward = ops.chrf_reward(strided(refs, extra), strided(hyps, 2 * extra), C.END, table, n, beta, counts=counts)
        runs.append((counts.cpu().numpy(), reward.cpu().numpy()))
    (got_counts, got), error = runs[0], np.abs(runs[0][1].astype(np.float64) - want)
    print("largest error", error.max(), "scores", got.tolist())
    assert all(c.tobytes() == got_counts.tobytes() and r.tobytes() == got.tobytes() for c, r in runs[1:])
    assert np.array_equal(got_counts, want_counts) and error.max() <= TOLERANCE and got.min() >= 0.0 and got.max() <= 1.0


@pytest.mark.parametrize("steps", [8, 33])
@pytest.mark.parametrize("samples", [1, 2, 3, 64])
def test_pairwise_utilities_layout_symmetry_and_diagonal(dev, samples, steps):
    from neuralmonkey_amd import ops
    from neuralmonkey_amd.decoders.mbr_decoder import tile_pairs
    from neuralmonkey_amd.trainers.self_critical_objective import SentenceChrF
    vocab, bsz, rng = C.vocabulary(), 1 if samples == 64 else 5, np.random.default_rng(steps * samples)
    words = np.array([C.A, C.AB, C.BAB, C.E_ACUTE, C.KANJI, C.AB_GLUE, C.B_GLUE], np.int32)
    tok = words[rng.integers(0, len(words), (steps, bsz, samples))]
    tok[rng.integers(steps), :, 0] = C.LONG_ID           # one sample of every sentence holds the 70-character word
    end = rng.integers(0, steps + 1, (bsz, samples))                             # == steps: the sample never ends
    end[0, 0], end[0, -1] = 0, steps
    tok[np.arange(steps)[:, None, None] >= end] = C.END
    pairs = tile_pairs(tok)                              # column (b n + i) n + j: reference sample j, hypothesis sample i
    for beta, join in ((1.0, True), (3.0, False)):
        table = SentenceChrF(vocab, 6, beta, None, join).device_table(dev)
        want = C.batch_scores(*pairs, vocab.index_to_word, 6, beta, (), join)[0].reshape(bsz, samples, samples)
        runs = [ops.chrf_pairwise(strided(tok, extra), C.END, table, 6, beta,
                                  out=torch.full((bsz, samples, samples), np.nan, device=dev)).cpu().numpy()
                for extra in (5, 5, 0)]
        got = runs[0]
        print("beta", beta, "largest error", np.abs(got - want).max())
        assert got.tobytes() == runs[1].tobytes() == runs[2].tobytes() and np.abs(got - want).max() <= TOLERANCE
        assert np.all(np.diagonal(got, axis1=1, axis2=2) == 1.0)
        assert np.array_equal(got, got.transpose(0, 2, 1)) == (beta == 1.0 or samples == 1)


def test_mbr_decoder_and_self_critical_rewards_end_to_end(dev, monkeypatch):
    """Both callers through ops.chrf_pairwise / ops.chrf_reward (counted) and, beyond a patched ops.chrf_max_chars(),
    through their host branches (tile_pairs counted, no further launch): the same choice, the same numbers."""
    from neuralmonkey_amd import ops
    from neuralmonkey_amd.decoders import MBRDecoder, mbr_decoder
    from neuralmonkey_amd.runtime import RunContext
    from neuralmonkey_amd.trainers import self_critical_objective as S
    from .test_mbr_decoder_gpu import _host, _mbr
    from .test_sampling_decoder_gpu import BATCH, PARENTS
    p, calls = PARENTS["rnn_fast"](dev), []
    for module, name in ((ops, "chrf_pairwise"), (ops, "chrf_reward"), (mbr_decoder, "tile_pairs")):
        monkeypatch.setattr(module, name, lambda *args, _inner=getattr(module, name), _name=name, **kw:
                            (calls.append(_name), _inner(*args, **kw))[1])
    words, chrf = p["dec"].vocabulary.index_to_word, S.SentenceChrF(p["dec"].vocabulary, beta=3.0)
    device, sampler = _mbr(p["dec"], name="mbr_chrf", utility=chrf)
    host = MBRDecoder("mbr_chrf_host", sampler, utility=chrf)
    objective, rng = S.SelfCriticalObjective(p["dec"], chrf), np.random.default_rng(3)
    refs, hyps = (rng.integers(2, 8, (t, BATCH)).astype(np.int32) for t in (9, 12))
    on_device = [torch.tensor(a, device=dev) for a in (refs, hyps)]
    ctx = RunContext(p["tfm"].sessions[0], p["fd"])                 # one context: both decoders see the same samples
    with torch.no_grad():
        fast, reward = _host(device.outputs(ctx)), objective.rewards(ctx, *on_device, "runtime").cpu().numpy()
        assert calls == ["chrf_pairwise", "chrf_reward"]
        monkeypatch.setattr(ops, "chrf_max_chars", lambda: 0)
        slow, reward_host = _host(host.outputs(ctx)), objective.rewards(ctx, *on_device, "train").cpu().numpy()
    assert calls == ["chrf_pairwise", "chrf_reward", "tile_pairs"]
    want = C.batch_scores(*mbr_decoder.tile_pairs(fast["samples"]), words, 6, 3.0)[0]
    assert np.array_equal(slow["samples"], fast["samples"]) and np.array_equal(fast["best"], slow["best"])
    assert np.array_equal(fast["tok"], slow["tok"]) and np.abs(fast["expected"] - slow["expected"]).max() <= TOLERANCE
    for got in (fast["utilities"], slow["utilities"]):
        assert np.abs(got.reshape(-1) - want).max() <= TOLERANCE
    for got in (reward, reward_host):
        assert np.abs(got - C.batch_scores(refs, hyps, words, 6, 3.0)[0]).max() <= TOLERANCE
    assert want.min() < 1.0 and reward.min() < reward.max()          # there was a choice to make, and rewards differ
