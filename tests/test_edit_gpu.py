"""nm_edit_reward and nm_edit_pairwise (csrc/nm_edit.hip) on the MI355X against the integer DP of tests/edit_ref.py, and
their two callers end to end.  Distances are integers and the finish rounds once from double: bytes are compared, no
tolerance.  Alphabets of 2 to 4 symbols; neighbouring columns of a batch hold pairs of sharply different lengths."""
import numpy as np
import pytest
import torch

from . import edit_ref as E
from . import mbr_ref as M

pytestmark = pytest.mark.gpu

KINDS = ("accuracy", "neg_wer")
# (T_hyp, T_ref, B): every W and C of the kernel and each boundary between them (16 | 17, 32 | 33, 64 | 65, C = 2, 4, 8, 16)
REWARD_SHAPES = [(1, 1024, 3), (16, 17, 5), (17, 16, 7), (32, 1, 3), (33, 40, 5), (64, 65, 3), (65, 64, 5), (129, 100, 3),
                 (300, 257, 1), (1024, 1024, 5), (1024, 7, 3)]


def batch(t_hyp, t_ref, bsz, seed):
    """Column b follows pattern (b + seed) % 7: no end token | an empty hypothesis | both empty | identical sentences |
    no common symbol | one reference token against a whole column | ends at random places."""
    rng = np.random.default_rng(seed)
    symbols, shorter = 2 + seed % 3, min(t_ref, t_hyp)
    refs = rng.integers(3, 3 + symbols, (t_ref, bsz)).astype(np.int32)
    hyps = rng.integers(3, 3 + symbols, (t_hyp, bsz)).astype(np.int32)
    hyps[:shorter, (3 - seed) % 7::7] = refs[:shorter, (3 - seed) % 7::7]
    hyps[:, (4 - seed) % 7::7] += symbols
    ends = [(None, None), (None, 0), (0, 0), (shorter - 1, shorter - 1), (None, None), (min(1, t_ref - 1), None),
            (rng.integers(t_ref), rng.integers(t_hyp))]               # </s> in (reference, hypothesis); None: never
    for b in range(bsz):
        for array, at in zip((refs, hyps), ends[(b + seed) % 7]):
            if at is not None:
                array[at, b] = E.END
    return refs, hyps


def strided(array, extra):
    """The array on the device with rows ``extra`` elements further apart than they need be; END in between."""
    wide = torch.full((array.shape[0], array[0].size + extra), E.END, dtype=torch.int32, device="cuda:0")
    wide[:, :array[0].size] = torch.tensor(array.reshape(array.shape[0], -1), device="cuda:0")
    return wide[:, :array[0].size].view(array.shape)


@pytest.mark.parametrize("t_hyp,t_ref,bsz", REWARD_SHAPES)
def test_reward_and_distance_are_the_integer_dp(dev, t_hyp, t_ref, bsz):
    from neuralmonkey_amd import ops
    refs, hyps = batch(t_hyp, t_ref, bsz, seed=t_hyp + bsz)
    d, lr, lh = E.distances(refs, hyps)
    for kind in KINDS:
        runs = []
        for extra in (3, 3, 0):                                                  # two equal runs; contiguous rows
            dist = torch.full((bsz,), -7, dtype=torch.int32, device=dev)
            reward = ops.edit_reward(kind, strided(refs, extra), strided(hyps, 2 * extra), E.END, dist=dist)
            runs.append((dist.cpu().numpy().tobytes(), reward.cpu().numpy().tobytes()))
        assert runs[0] == runs[1] == runs[2] == (d.tobytes(), E.score(kind, d, lr, lh).tobytes())


@pytest.mark.parametrize("steps", [8, 33, 130])
@pytest.mark.parametrize("n", [1, 2, 3, 64])
def test_pairwise_utilities_layout_symmetry_and_diagonal(dev, n, steps):
    from neuralmonkey_amd import ops
    from neuralmonkey_amd.decoders.mbr_decoder import tile_pairs
    from neuralmonkey_amd.trainers import self_critical_objective as S
    bsz, rng = 2 if n == 64 else 5, np.random.default_rng(steps * n)
    tok = rng.integers(3, 5 + n % 3, (steps, bsz, n)).astype(np.int32)
    end = rng.integers(0, steps + 1, (bsz, n))                                   # == steps: the sample never ends
    end[0, 0], end[0, -1] = 0, steps
    tok[np.arange(steps)[:, None, None] >= end] = E.END
    counts = E.distances(*tile_pairs(tok))              # column (b n + i) n + j: reference sample j, hypothesis sample i
    for kind, host in zip(KINDS, (S.sentence_edit_accuracy, S.sentence_neg_wer)):
        runs = [ops.edit_pairwise(kind, strided(tok, extra), E.END, out=torch.full((bsz, n, n), np.nan, device=dev))
                .cpu().numpy() for extra in (5, 5, 0)]
        got = runs[0]
        assert got.tobytes() == runs[1].tobytes() == runs[2].tobytes() == E.score(kind, *counts).tobytes()
        assert np.all(np.diagonal(got, axis1=1, axis2=2) == (1.0 if kind == "accuracy" else 0.0))
        if kind == "accuracy":
            assert np.array_equal(got, got.transpose(0, 2, 1)) and got.min() >= 0.0 and got.max() <= 1.0
        if n <= 3:                                                               # the host route's tiling: [b, i, j]
            assert got.tobytes() == host(*tile_pairs(tok)).tobytes()


def test_mbr_decoder_and_self_critical_rewards_end_to_end(dev, monkeypatch):
    """Both callers give the host functions' bits through ops.edit_pairwise / ops.edit_reward (counted), and through
    their host branches (tile_pairs counted, no further launch) beyond a patched ops.edit_max_tokens()."""
    from neuralmonkey_amd import ops
    from neuralmonkey_amd.decoders import MBRDecoder, mbr_decoder
    from neuralmonkey_amd.runtime import RunContext
    from neuralmonkey_amd.trainers import self_critical_objective as S
    from .test_mbr_decoder_gpu import _host, _mbr
    from .test_sampling_decoder_gpu import BATCH, PARENTS
    p, calls = PARENTS["rnn_fast"](dev), []
    for module, name in ((ops, "edit_pairwise"), (ops, "edit_reward"), (mbr_decoder, "tile_pairs")):
        monkeypatch.setattr(module, name, lambda *args, _inner=getattr(module, name), _name=name, **kw:
                            (calls.append(_name), _inner(*args, **kw))[1])
    short, sampler = _mbr(p["dec"], name="mbr_edit", utility=S.sentence_edit_accuracy)
    beyond = MBRDecoder("mbr_edit_beyond", sampler, utility=S.sentence_edit_accuracy)
    objective, rng = S.SelfCriticalObjective(p["dec"], S.sentence_neg_wer), np.random.default_rng(3)
    refs, hyps = (rng.integers(2, 6, (t, BATCH)).astype(np.int32) for t in (9, 12))
    on_device = [torch.tensor(a, device=dev) for a in (refs, hyps)]
    ctx = RunContext(p["tfm"].sessions[0], p["fd"])                 # one context: both decoders see the same samples
    with torch.no_grad():
        results = [_host(short.outputs(ctx))]
        rewards = [objective.rewards(ctx, *on_device, "runtime").cpu().numpy()]
        assert calls == ["edit_pairwise", "edit_reward"]
        monkeypatch.setattr(ops, "edit_max_tokens", lambda: 0)
        results.append(_host(beyond.outputs(ctx)))
        rewards.append(objective.rewards(ctx, *on_device, "train").cpu().numpy())
    assert calls == ["edit_pairwise", "edit_reward", "tile_pairs"]
    samples = results[0]["samples"]
    want = S.sentence_edit_accuracy(*mbr_decoder.tile_pairs(samples)).reshape(results[0]["utilities"].shape)
    expected, best, chosen, _ = M.select(want, samples)
    for r, reward in zip(results, rewards):
        assert reward.tobytes() == S.sentence_neg_wer(refs, hyps).tobytes()
        assert np.array_equal(r["samples"], samples) and r["utilities"].tobytes() == want.tobytes()
        assert r["expected"].tobytes() == expected.tobytes()
        assert np.array_equal(r["best"], best) and np.array_equal(r["tok"], chosen)
    assert want.min() < 1.0                                          # the samples differ: there was a choice to make
