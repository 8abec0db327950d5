"""The CPU restatement of the CTC head (tests/ctc_ref.py), which the GPU tests take as the expected value, against
independent formulations: exhaustive enumeration of every path in both merge modes (loss, and the gradient through
autograd of the enumeration), torch's CPU ctc_loss in float64 for the merging mode on ragged batches, hand-written
frame sequences for the greedy decoder, and the hand-off of its dense output to ``vectors_to_sentences``."""
import numpy as np
import pytest
import torch

from . import ctc_ref as R


def _cases():
    rng = np.random.default_rng(11)
    fixed = [(1, []), (3, []), (1, [0]), (2, [1, 1]), (3, [1, 1]), (4, [0, 0, 0]), (5, [2, 2]), (5, [0, 1, 0]),
             (2, [0, 1, 2]), (4, [1, 2, 2])]
    for frames, lab in fixed:
        yield frames, lab
    for _ in range(24):
        frames = int(rng.integers(1, 6))
        yield frames, [int(c) for c in rng.integers(0, 3, size=int(rng.integers(0, 4)))]


@pytest.mark.parametrize("merge", [True, False])
def test_loss_and_gradient_against_exhaustive_enumeration(merge):
    """4 classes (3 labels + blank), up to 5 frames: 4^5 paths at most.  Labels from empty to 3, repeats included;
    sentences without an alignment give loss 0 and gradient 0 in the restatement and no path in the enumeration."""
    rng = np.random.default_rng(5)
    seen_invalid = seen_repeat = seen_empty = 0
    for frames, lab in _cases():
        x = torch.tensor(rng.standard_normal((frames, 4)) * 2.0, dtype=torch.float64, requires_grad=True)
        want = R.brute_force_loss(torch.log_softmax(x, -1), lab, merge)
        loss, grad = R.sentence_loss_and_grad(x.detach().numpy(), lab, merge)
        seen_repeat += any(a == b for a, b in zip(lab, lab[1:]))
        seen_empty += not lab
        if want is None:
            seen_invalid += 1
            assert not R.has_alignment(lab, frames, merge), (frames, lab)
            assert loss == 0.0 and not grad.any()
            continue
        assert R.has_alignment(lab, frames, merge), (frames, lab)
        want.backward()
        assert abs(loss - want.item()) < 1e-11, (frames, lab, loss, want.item())
        assert np.abs(grad - x.grad.numpy()).max() < 1e-11, (frames, lab)
    assert seen_invalid >= 3 and seen_repeat >= 5 and seen_empty >= 3


def test_the_two_modes_differ_where_they_should():
    """[a, a] over two frames: one path without merging (a a), none with it (a blank is needed in between)."""
    x = np.zeros((2, 3))
    assert R.sentence_loss_and_grad(x, [0, 0], True)[0] == 0.0 and not R.has_alignment([0, 0], 2, True)
    loss, _ = R.sentence_loss_and_grad(x, [0, 0], False)
    assert abs(loss - 2 * np.log(3.0)) < 1e-12
    # [a] over two frames: merged 'a a', 'a -', '- a'; unmerged only 'a -', '- a' (no self-loop on a label)
    assert abs(R.sentence_loss_and_grad(x, [0], True)[0] + np.log(3 / 9.0)) < 1e-12
    assert abs(R.sentence_loss_and_grad(x, [0], False)[0] + np.log(2 / 9.0)) < 1e-12


def ragged_batch(seed, steps, bsz, classes, max_labels, dtype=np.float32, std=2.0):
    """Random logits [T, B, K], ragged frame lengths in [1, T] (sentence 0 full length) and label lists with repeats."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((steps, bsz, classes)) * std).astype(dtype)
    frame_lens = rng.integers(1, steps + 1, size=bsz).astype(np.int32)
    frame_lens[0] = steps
    labels = []
    for b in range(bsz):
        n = int(rng.integers(0, min(max_labels, int(frame_lens[b])) + 1))
        lab = rng.integers(0, classes - 1, size=n)
        if n > 2:
            lab[n // 2] = lab[n // 2 - 1]                      # a repeat
        labels.append([int(c) for c in lab])
    return logits, labels, frame_lens


@pytest.mark.parametrize("seed,steps,bsz,classes,max_labels", [(1, 13, 7, 5, 6), (2, 40, 5, 41, 12), (3, 9, 6, 3, 9)])
def test_merging_mode_against_torch_ctc_loss(seed, steps, bsz, classes, max_labels):
    logits, labels, frame_lens = ragged_batch(seed, steps, bsz, classes, max_labels, np.float64)
    x = torch.tensor(logits, requires_grad=True)
    flat = torch.tensor([c for lab in labels for c in lab], dtype=torch.long)
    want = torch.nn.functional.ctc_loss(torch.log_softmax(x, -1), flat, torch.tensor(frame_lens, dtype=torch.long),
                                        torch.tensor([len(lab) for lab in labels], dtype=torch.long), blank=classes - 1,
                                        reduction="none", zero_infinity=True)
    want.sum().backward()
    loss, grad = R.ctc_loss_and_grad(logits, labels, frame_lens, True)
    assert np.abs(loss - want.detach().numpy()).max() < 1e-9
    # (torch leaves NaN-free zeros for the sentences it calls infinite and for frames past the length)
    assert np.abs(grad - x.grad.numpy()).max() < 1e-9
    assert any(not R.has_alignment(lab, int(n), True) for lab, n in zip(labels, frame_lens)) or seed != 3
    for b in range(bsz):
        assert not grad[frame_lens[b]:, b].any()
    scaled = R.ctc_loss_and_grad(logits, labels, frame_lens, True, scale=0.25)[1]
    assert np.abs(scaled - 0.25 * grad).max() < 1e-15


def _frames(classes, k):
    """One-hot-ish logits [T, 1, k] whose argmax per frame is ``classes``."""
    x = np.zeros((len(classes), 1, k), np.float32)
    for t, c in enumerate(classes):
        x[t, 0, c] = 1.0
    return x


def test_greedy_decoder_on_hand_written_frames():
    a, b, blank = 0, 1, 2
    seq = [a, b, b, blank, b, blank, b]                         # the TF documentation's 'A B B * B * B'
    x = _frames(seq, 3)
    assert R.greedy(x, [7], True)[1] == [[a, b, b, b]]
    assert R.greedy(x, [7], False)[1] == [[a, b, b, b, b]]
    assert R.greedy(x, [3], True)[1] == [[a, b]]                # only the frames below the length count
    dense, outs = R.greedy(_frames([blank] * 4, 3), [4], True)
    assert outs == [[]] and dense.shape == (0, 1)              # a blank-only sequence emits nothing
    # ties go to the lowest class; a batch whose longest output sets the width, the rest padded with END
    tie = np.zeros((2, 1, 3), np.float32)
    assert R.greedy(tie, [2], True)[1] == [[0]] and R.greedy(tie, [2], False)[1] == [[0, 0]]
    batch = np.concatenate([_frames([a, blank, a, b], 3), _frames([blank, b, blank, blank], 3),
                            _frames([blank] * 4, 3)], axis=1)
    dense, outs = R.greedy(batch, [4, 4, 4], True)
    assert outs == [[a, a, b], [b], []]
    assert dense.tolist() == [[a, b, R.END], [a, R.END, R.END], [b, R.END, R.END]] and dense.dtype == np.int32


def test_dense_output_reaches_the_runner_as_sentences():
    """PlainRunner: vocabulary.vectors_to_sentences(list(decoded)); an all-END column is an empty sentence."""
    from neuralmonkey_amd.vocabulary import END_TOKEN_INDEX, Vocabulary
    assert R.END == END_TOKEN_INDEX
    vocab = Vocabulary(["yes", "no"])                           # ids 4, 5
    dense = np.array([[4, 5, END_TOKEN_INDEX], [5, END_TOKEN_INDEX, END_TOKEN_INDEX]], dtype=np.int32)
    assert vocab.vectors_to_sentences(list(dense)) == [["yes", "no"], ["no"], []]
    assert vocab.vectors_to_sentences(list(np.full((1, 2), END_TOKEN_INDEX, np.int32))) == [[], []]


def test_label_preparation():
    ids = np.array([[4, 4, 5, 0, 0], [5, 0, 0, 0, 0], [0, 0, 0, 0, 0], [4, 5, 5, 5, 4]])
    assert R.prepare_labels(ids, False) == [[4, 4, 5], [5], [], [4, 5, 5, 5, 4]]
    assert R.prepare_labels(ids, True) == [[4, 5], [5], [], [4, 5, 4]]
