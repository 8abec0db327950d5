"""CTC prefix beam search (csrc/nm_ctc_beam.hip) on the MI355X against ``beam_search_ref``, a float64 restatement of
include/nmhip_ctc_beam.h that enumerates all K - 1 extensions of every prefix (the kernel reads a row's beam_size + 1 best
classes).  Classes and lengths must be equal: every sentence of every case clears ``MARGIN`` between the last kept and the
first dropped candidate of every frame and between the two best final prefixes in float64 (asserted, nothing excluded;
tests/test_ctc_beam_host.py repeats it on the CPU).  Scores, as in tests/test_ctc_kernels_gpu.py: MULTIPLE units of the
float32 restatement's own error, capped at 1e-4 relative.  Largest unit: 3.4e-6 (k40_beam64, |score| 29)."""
import numpy as np
import pytest
import torch

from . import ctc_models as M
from .test_ctc_ref import ragged_batch

MULTIPLE, MARGIN, END, EPS32 = 16.0, 1e-4, 2, float(np.finfo(np.float32).eps)
# name -> (seed, T, B, K, beam_size, merge_repeated)
CASES = {"k3_beam4": (1, 13, 7, 3, 4, True), "k3_beam64": (2, 37, 5, 3, 64, False), "k5_beam4": (3, 13, 6, 5, 4, False),
         "k40_beam1_one_frame": (4, 1, 5, 40, 1, True), "k40_beam2": (5, 37, 5, 40, 2, False),
         "k40_beam16": (6, 13, 7, 40, 16, True), "k40_beam17": (14, 37, 6, 40, 17, False),
         "k40_beam64": (20, 37, 5, 40, 64, True), "k2003_beam8": (9, 13, 5, 2003, 8, True)}


def beam_search_ref(logits, frame_lens, beam_size, merge, dtype=np.float64):
    """(label lists, scores [B], smallest kept / dropped gap per sentence, best / second-best gap per sentence)."""
    bsz, blank, neg = logits.shape[1], logits.shape[2] - 1, dtype(-np.inf)
    outs, scores, cut_gaps, final_gaps = [], np.zeros(bsz, dtype), np.full(bsz, np.inf), np.full(bsz, np.inf)
    for b in range(bsz):
        beam = {(): (dtype(0.0), neg)}                               # prefix -> (pb, pl), in slot order
        for t in range(int(frame_lens[b])):
            x = logits[t, b].astype(dtype)
            lp = x - (x.max() + np.log(np.exp(x - x.max()).sum(dtype=dtype)))
            tot = {p: np.logaddexp(pb, pl) for p, (pb, pl) in beam.items()}
            survivors, ext = [], np.full((len(beam), blank), neg, dtype)
            for i, (p, (pb, pl)) in enumerate(beam.items()):
                new_pl = neg
                if p:
                    parent, prev = p[:-1], neg
                    if parent in beam:
                        prev = beam[parent][0] if parent and parent[-1] == p[-1] else tot[parent]
                    new_pl = lp[p[-1]] + np.logaddexp(pl, prev)
                survivors.append((tot[p] + lp[blank], new_pl))
                base = np.full(blank, tot[p], dtype)
                if p:
                    base[p[-1]] = pb
                ext[i] = lp[:blank] + base
                for q in beam:                                       # p + k that is in the beam already
                    if q and q[:-1] == p:
                        ext[i, q[-1]] = neg
            prefixes = list(beam)
            values = np.concatenate([np.array([np.logaddexp(a, c) for a, c in survivors], dtype), ext.ravel()])
            order = [j for j in np.argsort(-values, kind="stable")[:beam_size + 1] if values[j] > neg]
            if len(order) > beam_size:
                cut_gaps[b] = min(cut_gaps[b], float(values[order[beam_size - 1]]) - float(values[order[beam_size]]))
            beam = {}
            for j in order[:beam_size]:
                i, k = divmod(j - len(prefixes), blank)
                if j < len(prefixes):
                    beam[prefixes[j]] = survivors[j]
                else:
                    beam[prefixes[i] + (int(k),)] = (neg, values[j])
        best = ()
        if frame_lens[b] > 0:
            ranked = sorted(((np.logaddexp(pb, pl), i) for i, (pb, pl) in enumerate(beam.values())), reverse=True)
            best, scores[b] = list(beam)[ranked[0][1]], ranked[0][0]
            if len(ranked) > 1:
                final_gaps[b] = float(ranked[0][0]) - float(ranked[1][0])
        outs.append([c for i, c in enumerate(best) if not (merge and i > 0 and best[i - 1] == c)])
    return outs, scores, cut_gaps, final_gaps


def make_case(name):
    """(logits [T, B, K] float32 of standard deviation 3, frame lengths with a sentence of 0 and one of 1 frame)."""
    seed, steps, bsz, classes, _, _ = CASES[name]
    logits, _, frame_lens = ragged_batch(seed, steps, bsz, classes, 4, std=3.0)
    frame_lens[1], frame_lens[2] = 0, 1
    return logits, frame_lens


_EXPECTED = {}


def expectations(name):
    """The float64 result of a case and the bound on its scores; computed once."""
    if name not in _EXPECTED:
        logits, frame_lens = make_case(name)
        outs, score64, cut, final = beam_search_ref(logits, frame_lens, *CASES[name][4:])
        score32 = beam_search_ref(logits, frame_lens, *CASES[name][4:], np.float32)[1]
        mag = float(np.abs(score64).max())
        unit = max(float(np.abs(score32 - score64).max()), EPS32 * mag)
        _EXPECTED[name] = {"outs": outs, "score": score64, "cut_gap": cut, "final_gap": final,
                           "unit": unit, "bound": min(MULTIPLE * unit, 1e-4 * mag), "cap": 1e-4 * mag}
    return _EXPECTED[name]


def hand_made():
    """(a 0.4, blank 0.6) twice: greedy emits nothing (0.36), prefix 'a' sums to 0.64; a, blank, a at 0.9: 'a a'."""
    return (np.log(np.array([[[0.4, 0.6]], [[0.4, 0.6]]])).astype(np.float32),
            np.log(np.array([[[0.9, 0.1]], [[0.1, 0.9]], [[0.9, 0.1]]])).astype(np.float32))


def _run(dev, view, frame_lens, beam_size, merge):
    from neuralmonkey_amd import ops
    steps, bsz, _ = view.shape
    tokens = torch.full((bsz, steps), -7, dtype=torch.int32, device=dev)
    out_len = torch.full((bsz,), -7, dtype=torch.int32, device=dev)
    score = torch.full((bsz,), float("nan"), device=dev)
    ops.ctc_beam_search(view, torch.tensor(np.asarray(frame_lens, np.int32), device=dev), beam_size, merge, END, tokens,
                        out_len, score)
    torch.cuda.synchronize()
    return tokens.cpu().numpy(), out_len.cpu().numpy(), score.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_beam_search_against_float64(dev, name):
    """Also: two runs bit-equal; one case reads the transposed view of a batch-major product in a NaN-filled buffer."""
    logits, frame_lens = make_case(name)
    exp = expectations(name)
    steps, bsz, k = logits.shape
    assert exp["cut_gap"].min() > MARGIN and exp["final_gap"].min() > MARGIN, "choose inputs without near-ties"
    big = torch.full((bsz * steps + 2, k + 5), float("nan"), device=dev)
    big[1:1 + bsz * steps, 3:3 + k] = torch.tensor(np.ascontiguousarray(logits.transpose(1, 0, 2)).reshape(-1, k), device=dev)
    view = big.as_strided((steps, bsz, k), (k + 5, steps * (k + 5), 1), (k + 5) + 3)
    x = view if name == "k40_beam17" else torch.tensor(logits, device=dev)
    tokens, out_len, score = _run(dev, x, frame_lens, *CASES[name][4:])
    for b, want in enumerate(exp["outs"]):
        assert out_len[b] == len(want) and tokens[b, :out_len[b]].tolist() == want, (name, b)
        assert (tokens[b, out_len[b]:] == END).all(), (name, b)
    err = float(np.abs(score.astype(np.float64) - exp["score"]).max())
    print("{}: score error {:.3g} (unit {:.3g}, bound {:.3g})".format(name, err, exp["unit"], exp["bound"]))
    assert err <= exp["bound"] and out_len[1] == 0 and score[1] == 0.0            # no frame: nothing emitted, score 0
    again = _run(dev, x, frame_lens, *CASES[name][4:])
    assert all(np.array_equal(a, c) for a, c in zip((tokens, out_len, score), again))
    guard = torch.ones_like(big, dtype=torch.bool)
    guard[1:1 + bsz * steps, 3:3 + k] = False
    assert bool(torch.isnan(big[guard]).all()) and np.array_equal(x.cpu().numpy(), logits)


@pytest.mark.gpu
def test_prefix_merging_on_the_hand_made_cases(dev):
    from neuralmonkey_amd import ops
    two, aba = hand_made()
    tokens, out_len, score = _run(dev, torch.tensor(two, device=dev), [2], 4, True)
    assert out_len[0] == 1 and tokens[0, 0] == 0 and abs(float(score[0]) - np.log(0.64)) < 1e-6
    greedy, glen = torch.empty((1, 2), dtype=torch.int32, device=dev), torch.empty((1,), dtype=torch.int32, device=dev)
    ops.ctc_greedy(torch.tensor(two, device=dev), torch.tensor([2], dtype=torch.int32, device=dev), True, END, greedy, glen)
    assert int(glen[0]) == 0                                         # greedy decoding: blank, blank
    for merge, want in ((False, [0, 0]), (True, [0])):
        tokens, out_len, score = _run(dev, torch.tensor(aba, device=dev), [3], 4, merge)
        assert tokens[0, :out_len[0]].tolist() == want and abs(float(score[0]) - np.log(0.729)) < 1e-6


BEAM_INI = '\n[beam]\nclass=decoders.ctc_beam_search.CTCBeamSearchDecoder\nname="beam"\nparent_decoder=<decoder>\nbeam_size={}\n'


def load_wrapped(root, device, beam_size, **kw):
    from neuralmonkey_amd.config.configuration import load_experiment
    M.write_data(root, "speech")
    text = M.ini_text(root, "speech", **kw).replace("class=runners.PlainRunner\ndecoder=<decoder>",
                                                    "class=runners.PlainRunner\ndecoder=<beam>")
    (root / "beam.ini").write_text(text + BEAM_INI.format(beam_size))
    return load_experiment(str(root / "beam.ini"), device=str(device), seed=1234)


@pytest.mark.gpu
@pytest.mark.parametrize("beam_size", [1, 5])
def test_decoder_through_plain_runner(dev, tmp_path, beam_size):
    """The sentences the restatement decodes from the parent's fetched logits (beam 1 is not greedy decoding)."""
    from neuralmonkey_amd.runtime import RunContext
    model = load_wrapped(tmp_path, dev, beam_size)
    runner, sess = model.runners[0], model.tf_manager.sessions[0]
    wrapper, parent = runner.decoder, runner.decoder.parent_decoder
    sess.store["decoder/state_to_word_W"].mul_(4.0)                  # peaked frames: beams that do not collapse into ties
    sess.store["decoder/state_to_word_b"].add_(torch.linspace(-1.0, 1.0, 8, device=dev))
    sess.variables_changed()
    batch = next(iter(model.train_dataset.batches()))
    out = model.tf_manager.execute(batch, runner.feedables, [runner])[0]
    ctx = RunContext(sess, {k: v for part in runner.feedables for k, v in part.feed_dict(batch, train=False).items()})
    want, score, cut, final = beam_search_ref(parent.logits(ctx).cpu().numpy(), parent.frame_lengths(ctx).cpu().numpy(),
                                              beam_size, wrapper.merge_repeated_outputs)
    assert cut.min() > MARGIN and final.min() > MARGIN
    assert out.outputs["target"] == [[wrapper.vocabulary.index_to_word[c] for c in s] for s in want]
    assert np.abs(wrapper.scores(ctx).cpu().numpy() - score).max() <= 1e-4 * np.abs(score).max()
    assert out.losses["target/train_loss"] == out.losses["target/runtime_loss"] > 0.0
