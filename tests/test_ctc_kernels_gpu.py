"""The CTC kernels (csrc/nm_ctc.hip) called directly through ``ops`` on the MI355X against tests/ctc_ref.py in float64.

Cases (``CASES``): both merge modes; K = V + 1 of 3, 40 and 32001; T and B that are multiples of nothing; ragged frame
and label lengths in one batch; in every batch a sentence with no label (L = 0), one with a single frame, one without
an alignment (more labels than frames: loss and gradient exactly 0) and repeated labels; 2L + 1 = 1041 states, above
the workgroup's 1024 threads; labels that went through ``merge_repeated_targets``; logits as a strided slice of a
NaN-filled buffer (the guard elements must still be NaN) and as the transposed view of a batch-major product;
``scale`` from a device scalar; the gradient in place and out of place; two runs bit-equal.

Tolerances (the method of tests/test_pointwise_refs.py): the UNIT is the error of the float32 NumPy evaluation of the
restatement against its float64 evaluation on the case's own inputs (never below one float32 epsilon of the largest
magnitude); the kernel is allowed ``MULTIPLE`` = 16 units, because its sums run in other orders (64-lane trees for the
row log-sum-exps, a chain over the frames whose three-term sums it orders by magnitude) and its exp / log are the
hardware's v_exp_f32 / v_log_f32 (1 ulp, plus the rounding of the argument's product with log2 e, which grows with the
argument).  The bound never exceeds what smoke() allows: 1e-4 relative on a loss, 1e-3 of the largest magnitude on a
gradient.  tests/test_ctc_host.py checks on the CPU that these bounds are positive, under the caps, and that no frame
of any case has a top-two gap within the greedy comparison's exclusion margin."""
import numpy as np
import pytest
import torch

from . import ctc_ref as R
from .test_ctc_ref import ragged_batch

MULTIPLE = 16.0
EPS32 = float(np.finfo(np.float32).eps)
HERE = "tests/test_ctc_kernels_gpu.py::"

# name -> (seed, T, B, K, longest label sequence, merge_repeated_outputs, collapse repeated targets first)
CASES = {
    "k3_merge": (1, 13, 7, 3, 6, True, False),
    "k3_plain": (2, 13, 7, 3, 6, False, False),
    "k40_merge": (3, 37, 5, 40, 12, True, False),
    "k40_plain": (4, 37, 5, 40, 12, False, False),
    "k40_collapsed_targets": (5, 29, 6, 40, 14, True, True),
    "vocab_merge": (6, 11, 5, 32001, 5, True, False),
    "vocab_plain": (7, 11, 5, 32001, 5, False, False),
    "states_above_the_workgroup": (8, 613, 4, 3, 520, False, False),
}


def make_case(name):
    """(logits [T, B, K] float32, label lists, frame lengths): a ragged random batch whose sentences 1..3 are the
    special ones -- no label, one frame, more labels than frames."""
    seed, steps, bsz, classes, max_labels, merge, collapse = CASES[name]
    logits, labels, frame_lens = ragged_batch(seed, steps, bsz, classes, max_labels)
    rng = np.random.default_rng(seed + 100)
    if max_labels > 100:                               # sentence 0: all T frames, 520 labels -> 1041 states
        labels[0] = [int(c) for c in rng.integers(0, classes - 1, size=max_labels)]
    labels[1] = []
    frame_lens[2], labels[2] = 1, [int(rng.integers(0, classes - 1))]
    frame_lens[3], labels[3] = 2, [0, 1 % (classes - 1), 0]
    if collapse:
        ids = np.zeros((bsz, max(len(l) for l in labels) + 1), np.int32)
        for b, lab in enumerate(labels):
            ids[b, :len(lab)] = np.asarray(lab) + 1            # 0 is <pad>: shift the classes up by one
        from neuralmonkey_amd.decoders.ctc_decoder import prepare_labels
        arr, lens = prepare_labels(ids, True)
        assert R.prepare_labels(ids, True) == [list(arr[b, :lens[b]]) for b in range(bsz)]
        assert any(lens[b] < len(labels[b]) for b in range(bsz)), "no repeated target to collapse"
        labels = [[int(c) - 1 for c in arr[b, :lens[b]]] for b in range(bsz)]
    return logits, labels, frame_lens, merge


def expectations(name, scale=1.0):
    """float64 loss / gradient and the bounds the kernel is held to."""
    logits, labels, frame_lens, merge = make_case(name)
    loss64, grad64 = R.ctc_loss_and_grad(logits, labels, frame_lens, merge, np.float64, scale)
    loss32, grad32 = R.ctc_loss_and_grad(logits, labels, frame_lens, merge, np.float32, scale)
    lmag, gmag = float(np.abs(loss64).max()), float(np.abs(grad64).max())
    unit_loss = max(float(np.abs(loss32 - loss64).max()), EPS32 * lmag)
    unit_grad = max(float(np.abs(grad32 - grad64).max()), EPS32 * gmag)
    return {"loss": loss64, "grad": grad64, "unit_loss": unit_loss, "unit_grad": unit_grad,
            "bound_loss": min(MULTIPLE * unit_loss, 1e-4 * lmag), "bound_grad": min(MULTIPLE * unit_grad, 1e-3 * gmag),
            "cap_loss": 1e-4 * lmag, "cap_grad": 1e-3 * gmag}


def greedy_margin(logits):
    """Frames whose float64 top-two gap is within this margin are left out of the greedy comparison: the kernel reads
    the same float32 logits the restatement reads, so only an exact tie could differ -- one float32 epsilon of the
    largest logit is already generous."""
    return EPS32 * float(np.abs(logits).max())


def _device_labels(labels, dev):
    lmax = max([len(l) for l in labels] + [0])
    arr = np.zeros((len(labels), lmax), np.int32)
    for b, lab in enumerate(labels):
        arr[b, :len(lab)] = lab
    return (torch.tensor(arr, device=dev), torch.tensor([len(l) for l in labels], dtype=torch.int32, device=dev))


def _run(dev, logits_view, labels, frame_lens, merge, scale=None, out=None):
    """ops.ctc_loss_fwd + ops.ctc_loss_bwd on a [T, B, K] device view; ``out`` None: in place."""
    from neuralmonkey_amd import ops
    lab, lab_len = _device_labels(labels, dev)
    flen = torch.tensor(np.asarray(frame_lens, np.int32), device=dev)
    bsz = logits_view.shape[1]
    loss = torch.full((bsz,), float("nan"), device=dev)
    total = torch.full((1,), float("nan"), device=dev)
    ws = ops.ctc_loss_fwd(logits_view, lab, lab_len, flen, merge, loss, total)
    sc = None if scale is None else torch.tensor([scale], device=dev)
    grad = ops.ctc_loss_bwd(logits_view, lab, lab_len, flen, logits_view if out is None else out, ws, sc)
    torch.cuda.synchronize()
    return loss.cpu().numpy().astype(np.float64), float(total.cpu()[0]), grad.cpu().numpy().astype(np.float64)


def _check(name, exp, loss, total, grad, labels, frame_lens, merge):
    err_loss = float(np.abs(loss - exp["loss"]).max())
    err_grad = float(np.abs(grad - exp["grad"]).max())
    print("{}: loss error {:.3g} (unit {:.3g}, bound {:.3g}), gradient error {:.3g} (unit {:.3g}, bound {:.3g})".format(
        name, err_loss, exp["unit_loss"], exp["bound_loss"], err_grad, exp["unit_grad"], exp["bound_grad"]))
    assert err_loss <= exp["bound_loss"], (name, err_loss, exp["bound_loss"])
    assert abs(total - exp["loss"].sum()) <= len(loss) * exp["bound_loss"], name
    assert err_grad <= exp["bound_grad"], (name, err_grad, exp["bound_grad"])
    for b, (lab, n) in enumerate(zip(labels, frame_lens)):
        assert not grad[n:, b].any(), (name, b, "frames past the length")          # exact zeros
        if not R.has_alignment(lab, int(n), merge):
            assert loss[b] == 0.0 and not grad[:, b].any(), (name, b, "no alignment")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_loss_and_gradient_in_place(dev, name):
    logits, labels, frame_lens, merge = make_case(name)
    exp = expectations(name)
    assert any(not R.has_alignment(l, int(n), merge) for l, n in zip(labels, frame_lens))
    x = torch.tensor(logits, device=dev)
    loss, total, grad = _run(dev, x, labels, frame_lens, merge)
    _check(name, exp, loss, total, grad, labels, frame_lens, merge)
    # two runs on the same inputs are bit-equal (no floating-point atomics anywhere)
    x2 = torch.tensor(logits, device=dev)
    loss2, total2, grad2 = _run(dev, x2, labels, frame_lens, merge)
    assert np.array_equal(loss, loss2) and total == total2 and np.array_equal(grad, grad2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["k40_merge", "k3_plain"])
def test_strided_logits_scale_and_out_of_place_gradient(dev, name):
    """The logits are a slice of a NaN-filled buffer, the gradient goes to a slice of another; every guard element of
    both is still NaN afterwards, the logits are untouched, ``scale`` multiplies the gradient."""
    logits, labels, frame_lens, merge = make_case(name)
    steps, bsz, k = logits.shape
    scale = 0.37
    exp = expectations(name, scale)
    big = torch.full((steps + 1, bsz + 2, k + 5), float("nan"), device=dev)
    view = big[:steps, 1:1 + bsz, 3:3 + k]
    view.copy_(torch.tensor(logits, device=dev))
    out_big = torch.full((steps, bsz + 1, k + 3), float("nan"), device=dev)
    out = out_big[:, 1:, 1:1 + k]
    loss, total, grad = _run(dev, view, labels, frame_lens, merge, scale=scale, out=out)
    _check(name, exp, loss, total, grad, labels, frame_lens, merge)
    assert np.array_equal(view.cpu().numpy(), logits)
    guard = torch.ones_like(big, dtype=torch.bool)
    guard[:steps, 1:1 + bsz, 3:3 + k] = False
    assert bool(torch.isnan(big[guard]).all())
    guard = torch.ones_like(out_big, dtype=torch.bool)
    guard[:, 1:, 1:1 + k] = False
    assert bool(torch.isnan(out_big[guard]).all()) and not bool(torch.isnan(out).any())
    # the decoder's layout: a batch-major product [B*T, K] read as [T, B, K], gradient in place
    bm = torch.tensor(np.ascontiguousarray(logits.transpose(1, 0, 2)), device=dev)
    loss_t, total_t, grad_t = _run(dev, bm.transpose(0, 1), labels, frame_lens, merge, scale=scale)
    _check(name, exp, loss_t, total_t, grad_t, labels, frame_lens, merge)
    assert np.array_equal(loss_t, loss)                  # the same arithmetic whatever the strides


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_greedy_decoding(dev, name):
    from neuralmonkey_amd import ops
    logits, _, frame_lens, _ = make_case(name)
    steps, bsz, k = logits.shape
    gap = R.top_two_gap(logits)
    unsure = gap <= greedy_margin(logits)
    assert unsure.mean() <= 0.01 and not unsure.any(), "choose inputs without near-ties"
    x = torch.tensor(logits, device=dev)
    flen = torch.tensor(frame_lens, device=dev)
    for merge in (True, False):
        tokens = torch.full((bsz, steps), -7, dtype=torch.int32, device=dev)
        out_len = torch.full((bsz,), -7, dtype=torch.int32, device=dev)
        ops.ctc_greedy(x, flen, merge, R.END, tokens, out_len)
        torch.cuda.synchronize()
        _, want = R.greedy(logits, frame_lens, merge)
        got, lens = tokens.cpu().numpy(), out_len.cpu().numpy()
        for b in range(bsz):
            assert lens[b] == len(want[b]) and got[b, :lens[b]].tolist() == want[b], (name, merge, b)
            assert (got[b, lens[b]:] == R.END).all()                       # pre-filled with END up to T
    assert np.array_equal(x.cpu().numpy(), logits)


@pytest.mark.gpu
def test_greedy_documentation_case_ties_and_mask_lengths(dev):
    """'A B B * B * B' -> A B B B merged, A B B B B unmerged; a blank-only sentence; ties go to the lowest class; the
    frame lengths as int32 row sums of a float mask."""
    from neuralmonkey_amd import ops
    a, b, blank = 0, 1, 2
    seqs = [[a, b, b, blank, b, blank, b], [blank] * 7, [b, b, b, b, a, a, blank]]
    x = np.zeros((7, 4, 3), np.float32)                  # sentence 3: all ties -> class 0 every frame
    for s, seq in enumerate(seqs):
        for t, c in enumerate(seq):
            x[t, s, c] = 1.0
    mask = np.zeros((4, 7), np.float32)
    for s, n in enumerate([7, 7, 6, 5]):
        mask[s, :n] = 1.0
    flen = ops.ctc_mask_lengths(torch.tensor(mask, device=dev))
    assert flen.dtype == torch.int32 and flen.cpu().tolist() == [7, 7, 6, 5]
    for merge, want in ((True, [[a, b, b, b], [], [b, a], [a]]), (False, [[a, b, b, b, b], [], [b, b, b, b, a, a], [a] * 5])):
        tokens = torch.empty((4, 7), dtype=torch.int32, device=dev)
        out_len = torch.empty((4,), dtype=torch.int32, device=dev)
        ops.ctc_greedy(torch.tensor(x, device=dev), flen, merge, R.END, tokens, out_len)
        got, lens = tokens.cpu().numpy(), out_len.cpu().tolist()
        assert [got[s, :lens[s]].tolist() for s in range(4)] == want
        assert R.greedy(x, [7, 7, 6, 5], merge)[1] == want


@pytest.mark.gpu
def test_autodiff_op_overwrites_the_logits_with_their_gradient(dev):
    """autodiff.ctc_loss on a recording tape: batch-major logits [B*T, K] become grad_scale * d sum / d logits."""
    from neuralmonkey_amd import autodiff as F
    name = "k40_merge"
    logits, labels, frame_lens, merge = make_case(name)
    exp = expectations(name, 0.5)
    steps, bsz, k = logits.shape

    class Ctx:                                            # what a Tape asks of a run context (no session: no arena)
        device = None
        bufs = {}

        def buffer(self, key, shape, dtype=torch.float32, zero=False, zero_init=False):
            return self.bufs.setdefault((key, tuple(shape), dtype), torch.zeros(tuple(shape), dtype=dtype, device=dev))

    F_tape = F.Tape(Ctx(), "ctc_test", recording=True)
    var = F_tape.leaf(torch.tensor(np.ascontiguousarray(logits.transpose(1, 0, 2)).reshape(bsz * steps, k), device=dev),
                      needs_grad=True)
    lab, lab_len = _device_labels(labels, dev)
    loss, total = F.ctc_loss(F_tape, var, bsz, steps, lab, lab_len, torch.tensor(frame_lens, device=dev), merge,
                             torch.tensor([0.5], device=dev))
    torch.cuda.synchronize()
    assert var.grad is var.data
    grad = var.grad.view(bsz, steps, k).transpose(0, 1).cpu().numpy().astype(np.float64)
    _check(name, exp, loss.cpu().numpy().astype(np.float64), float(total.cpu()[0]), grad, labels, frame_lens, merge)


# each entry point of include/nmhip_ctc.h -> the test above that calls it (the rules of
# tests/test_pointwise_refs.py::ledger_problems; checked in tests/test_ctc_host.py)
LEDGER = {
    "nm_ctc_workspace_bytes": ("no kernel", "plain arithmetic on the three sizes; every test above sizes its workspace "
                                            "with it through ops.ctc_workspace"),
    "nm_ctc_mask_lengths": HERE + "test_greedy_documentation_case_ties_and_mask_lengths via ops.ctc_mask_lengths",
    "nm_ctc_loss_fwd": HERE + "test_loss_and_gradient_in_place via ops.ctc_loss_fwd",
    "nm_ctc_loss_bwd": HERE + "test_loss_and_gradient_in_place via ops.ctc_loss_bwd",
    "nm_ctc_greedy": HERE + "test_greedy_decoding via ops.ctc_greedy",
}
