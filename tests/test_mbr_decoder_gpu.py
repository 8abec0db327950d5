"""MBRDecoder over ``SamplingDecoder(num_samples=8)`` with an RNN parent and a Transformer parent (the small synthetic
models of tests/test_sampling_decoder_gpu.py: B = 6, V = 300, width 32, at most 10 steps).

The chosen sentence is the column ``best[b]`` of the decoder's own samples; ``utilities``, ``expected_utility`` and
``best`` are the host oracle's (tests/mbr_ref.py) on those samples -- GLEU bit for bit, BLEU within one float32 unit in
the last place with its select step bit-equal on the device's own utilities; a session rebuilt with the same seed
reproduces everything; a host callable that wraps ``sentence_gleu`` goes through the tiled pairs and ``nm_mbr_select``
to the same choice; the runner emits the chosen samples cut at </s> with the mean expected utility of the chosen
samples as its loss; and the path launches no ``at::native`` kernel."""
import numpy as np
import pytest
import torch

from . import mbr_ref as M
from .test_sampling_decoder_gpu import BATCH, PARENTS, STEPS, _sampler

pytestmark = pytest.mark.gpu

SAMPLES = 8


def _mbr(parent, name="mbr", **kw):
    from neuralmonkey_amd.decoders import MBRDecoder
    sampler = _sampler(parent, name=name + "_sampler", num_samples=SAMPLES)
    return MBRDecoder(name, sampler, **kw), sampler


def _host(out):
    pull = lambda t: t.detach().cpu().numpy().copy()
    return dict(tok=pull(out.token_ids), best=pull(out.best), expected=pull(out.expected_utility),
                utilities=pull(out.utilities), samples=pull(out.samples.token_ids), lps=pull(out.samples.logprob_sum))


def _run(sess, fd, *decoders):
    """The outputs of several MBR decoders in ONE run context: decoders over one sampler share its samples."""
    from neuralmonkey_amd.runtime import RunContext
    ctx = RunContext(sess, fd)
    with torch.no_grad():
        results = [_host(d.outputs(ctx)) for d in decoders]
    return results


def _check_against_oracle(res, kind):
    samples = res["samples"]
    steps, bsz, n = samples.shape
    assert (bsz, n) == (BATCH, SAMPLES) and 1 <= steps <= STEPS
    assert res["tok"].shape == (steps, bsz) and res["best"].shape == (bsz,) and res["best"].dtype == np.int32
    assert res["expected"].shape == (bsz, n) and res["utilities"].shape == (bsz, n, n)
    for b in range(bsz):
        assert np.array_equal(res["tok"][:, b], samples[:, b, res["best"][b]]), b
    want = M.pairwise(kind, samples)
    if kind == "gleu":
        assert np.array_equal(res["utilities"], want)
        utilities = want
    else:
        assert M.ulps(res["utilities"], want).max() <= 1 and np.array_equal(res["utilities"] == 0, want == 0)
        utilities = res["utilities"]
    expected, best, chosen, _ = M.select(utilities, samples)
    assert res["expected"].tobytes() == expected.tobytes()
    assert np.array_equal(res["best"], best) and np.array_equal(res["tok"], chosen)
    return best


@pytest.mark.parametrize("parent", ["rnn_fast", "transformer"])
def test_mbr_decoder_against_the_oracle(dev, parent):
    from neuralmonkey_amd.trainers.self_critical_objective import sentence_bleu, sentence_gleu
    p = PARENTS[parent](dev)
    gleu, sampler = _mbr(p["dec"])
    from neuralmonkey_amd.decoders import MBRDecoder
    bleu = MBRDecoder("mbr_bleu", sampler, utility=sentence_bleu)
    calls = []

    def wrapped(references, hypotheses):                  # not the function object: the host route
        calls.append((references.shape, hypotheses.shape))
        return sentence_gleu(references, hypotheses)
    host = MBRDecoder("mbr_host", sampler, utility=wrapped)
    sess = p["tfm"].sessions[0]
    res_gleu, res_bleu, res_host = _run(sess, p["fd"], gleu, bleu, host)
    steps = res_gleu["samples"].shape[0]
    for other in (res_bleu, res_host):                    # one run context: the decoders share the sampler's samples
        assert np.array_equal(res_gleu["samples"], other["samples"])
    best = _check_against_oracle(res_gleu, "gleu")
    _check_against_oracle(res_bleu, "bleu")
    print(parent, "steps", steps, "best (GLEU)", best.tolist(), "best (BLEU)", res_bleu["best"].tolist())
    for b in range(BATCH):                                # the samples of a sentence differ: there is a choice to make
        assert len({tuple(res_gleu["samples"][:, b, j]) for j in range(SAMPLES)}) > 1, b
    # the host callable: called once over the B * n * n tiled pairs, the same utilities, the same choice
    assert calls == [((steps, BATCH * SAMPLES * SAMPLES),) * 2]
    assert np.array_equal(res_host["utilities"], res_gleu["utilities"])
    assert np.array_equal(res_host["best"], res_gleu["best"]) and np.array_equal(res_host["tok"], res_gleu["tok"])
    assert res_host["expected"].tobytes() == res_gleu["expected"].tobytes()
    # a session rebuilt with the same seed reproduces the run
    q = PARENTS[parent](dev)
    again, _ = _mbr(q["dec"])
    res_again, = _run(q["tfm"].sessions[0], q["fd"], again)
    for key in ("samples", "lps", "utilities", "expected", "best", "tok"):
        assert res_again[key].tobytes() == res_gleu[key].tobytes(), key
    # ... and the same session draws afresh, and chooses among the new samples
    res_next, = _run(sess, p["fd"], gleu)
    first, second = res_gleu["samples"], res_next["samples"]
    assert second.shape != first.shape or not np.array_equal(second, first)
    _check_against_oracle(res_next, "gleu")


def test_runner_sentences_are_the_cut_choice_and_the_loss_is_its_mean_utility(dev):
    from neuralmonkey_amd.runners import MBRRunner
    a = PARENTS["rnn_fast"](dev)
    decoder, _ = _mbr(a["dec"])
    runner = MBRRunner("target_mbr", decoder)
    got = a["tfm"].execute(a["ds"], runner.feedables, [runner])[0]
    b = PARENTS["rnn_fast"](dev)                          # the same seed: the same draws
    again, _ = _mbr(b["dec"])
    res, = _run(b["tfm"].sessions[0], b["fd"], again)
    vocab = b["dec"].vocabulary
    assert got.outputs["target_mbr"] == vocab.vectors_to_sentences(res["tok"])
    for sentence in got.outputs["target_mbr"]:
        assert "</s>" not in sentence and "<pad>" not in sentence
    assert set(got.losses) == {"target_mbr/expected_utility"}
    want = float(np.mean(res["expected"][np.arange(BATCH), res["best"]]))
    assert abs(got.losses["target_mbr/expected_utility"] - want) < 1e-6
    assert 0.0 < want <= 1.0 and got.size == BATCH
    shouted = MBRRunner("target_mbr", decoder, postprocess=lambda sentences: [[w.upper() for w in s] for s in sentences])
    loud = a["tfm"].execute(a["ds"], shouted.feedables, [shouted], compute_losses=False)[0]
    assert all(w == w.upper() for s in loud.outputs["target_mbr"] for w in s)


def test_mbr_decoding_launches_no_torch_kernels(dev):
    from neuralmonkey_amd.runners import MBRRunner
    from tests.test_no_foreign_kernels_gpu import _foreign_kernels
    p = PARENTS["rnn_fast"](dev)
    decoder, _ = _mbr(p["dec"])
    runner = MBRRunner("target_mbr", decoder)
    foreign = _foreign_kernels(lambda: p["tfm"].execute(p["ds"], runner.feedables, [runner], compute_losses=False))
    assert not foreign, foreign
