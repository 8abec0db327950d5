"""The labelling-head kernels (csrc/nm_label.hip) called through ``ops.label_rows`` on the MI355X against
tests/label_ref.py in float64.

Cases (``CASES``): (rows, K) = (5, 1), (7, 2), (133, 43) with a leading dimension of 48, (9, 64), (9, 65), (6, 257),
(5, 1024) -- one and two classes, the reference's tag set, both sides of every register-count step of the packed kernel
(64 | 65, 256 | 257), its widest row -- and (3, 1028), which goes through the vocabulary-row kernels with the same
expectations.  Every case holds a row of equal values (argmax 0), a row whose target is the pad id (loss and gradient
exactly 0), a row with ``row_mask`` 0 but a real target (its loss counts, its label is the masked class), rows shifted
by +80 and by -80, a row shifted by +100 (and, from five rows on, one by -110: without the maximum subtracted their
exponentials overflow / all underflow in float32, which +-80 do not) and a row with a -inf class that is not the target
(K = 1 has no such class); with few rows a row carries several of these.
At K < 3 class 0 cannot double as the pad id, which is -1 there.

Tolerances (the method of tests/test_pointwise_refs.py / test_ctc_kernels_gpu.py): the UNIT is the error of the float32
NumPy evaluation of the restatement against its float64 evaluation on the case's own inputs, never below one float32
epsilon of the largest magnitude; the kernel is allowed ``MULTIPLE`` = 16 units (its sums run as 64-lane trees, its
exp / log are the device library's), never more than smoke()'s caps: 1e-4 relative on a loss, 1e-3 of the largest
magnitude on a gradient, 1e-4 of the largest magnitude on the log-probabilities.  At K = 1 every output is identically
zero in float64 AND in float32 (log 1, 1 - 1): unit and bound are 0 and the kernel has to be exact.  Argmax and labels
are compared on every row: the kernel reads the float32 logits the restatement reads, so only an exact tie could
differ, and the only exact ties are the rows of equal values, whose answer (class 0) is asserted; tests/
test_labeler_host.py checks that no other row's top-two gap is within one float32 epsilon of its largest magnitude."""
import numpy as np
import pytest
import torch

from . import label_ref as R

MULTIPLE = 16.0
EPS32 = float(np.finfo(np.float32).eps)
HERE = "tests/test_label_kernels_gpu.py::"
MASKED = R.END

# name -> (seed, rows, K, leading dimension)
CASES = {
    "k1": (1, 5, 1, 1),
    "k2": (2, 7, 2, 2),
    "k43_ld48": (3, 133, 43, 48),
    "k64": (4, 9, 64, 64),
    "k65": (5, 9, 65, 65),
    "k257": (6, 6, 257, 257),
    "k1024": (7, 5, 1024, 1024),
    "k1028_fallback": (8, 3, 1028, 1028),
}


def pad_id_of(k):
    return 0 if k >= 3 else -1


def special_rows(rows):
    """Which rows carry which property.  The shifts double up with the other properties so that EVERY case holds a
    row at +80 and one at -80 (which float32 still exponentiates without the maximum subtracted) and a row at +100
    (exp overflows without it); from five rows on also one at -110 (every exponential underflows to 0 without it)."""
    if rows >= 5:
        where = {"equal": 0, "pad": 1, "masked": 2, "up": 3, "ninf": 4, "over": 2, "under": 1,
                 "down": rows - 1 if rows >= 6 else 0}
    else:
        where = {"equal": 0, "masked": 0, "down": 0, "pad": 1, "up": 1, "ninf": 2, "over": 2}
    return where


SHIFTS = {"up": 80.0, "down": -80.0, "over": 100.0, "under": -110.0}


def make_case(name):
    """(logits [rows, K] float32, targets [rows] int32, row_mask [rows] float32, pad id)."""
    seed, rows, k, _ = CASES[name]
    rng = np.random.default_rng(seed)
    pad = pad_id_of(k)
    x = (1.5 * rng.standard_normal((rows, k))).astype(np.float32)
    real = np.arange(1, k) if pad == 0 else np.arange(k)
    t = rng.choice(real, size=rows).astype(np.int32)
    mask = np.ones(rows, np.float32)
    mask[rng.random(rows) < 0.2] = 0.0
    where = special_rows(rows)
    x[where["equal"]] = 0.25
    t[where["pad"]] = pad
    mask[where["masked"]] = 0.0
    for prop, shift in SHIFTS.items():
        if prop in where:
            x[where[prop]] += np.float32(shift)
    if k > 1:
        r = where["ninf"]
        others = [c for c in range(k) if c != t[r]]
        x[r, others[:: max(1, len(others) // 3)]] = -np.inf
    return x, t, mask, pad


def _mag(a):
    a = np.asarray(a, np.float64)
    fin = a[np.isfinite(a)]
    return float(np.abs(fin).max()) if fin.size else 0.0


def _err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin]), "non-finite entries differ"
    return float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0


def expectations(name, scale=1.0):
    """float64 outputs and the bounds the kernel is held to."""
    x, t, mask, pad = make_case(name)
    r64 = R.rows(x, t, pad, scale, np.float64, mask, MASKED)
    r32 = R.rows(x, t, pad, scale, np.float32, mask, MASKED)
    exp = dict(r64)
    for key, cap in (("loss", 1e-4), ("grad", 1e-3), ("logprobs", 1e-4)):
        mag = _mag(r64[key])
        unit = max(_err(r32[key], r64[key]), EPS32 * mag)
        exp["unit_" + key], exp["cap_" + key] = unit, cap * mag
        exp["bound_" + key] = min(MULTIPLE * unit, cap * mag)
    return exp


def argmax_margin(x):
    """Rows whose float64 top-two gap is within this margin could differ in argmax: one float32 epsilon of the row's
    largest (finite) magnitude."""
    mags = np.array([_mag(row) for row in x])
    return EPS32 * mags


def _run(dev, name, scale=None, offset=(0, 0), with_targets=True, logprobs=True):
    """One ``ops.label_rows`` call asking for everything, the logits a slice of a NaN-filled buffer."""
    from neuralmonkey_amd import ops
    x, t, mask, pad = make_case(name)
    _, rows, k, ld = CASES[name]
    r0, c0 = offset
    big = torch.full((rows + 2 * r0, ld + 2 * c0), float("nan"), device=dev)
    view = big[r0:r0 + rows, c0:c0 + k]
    view.copy_(torch.tensor(x, device=dev))
    lp_big = torch.full((rows + r0, k + 3 + c0), float("nan"), device=dev)
    lp = lp_big[r0:, c0:c0 + k]
    loss = torch.full((rows,), float("nan"), device=dev)
    amax = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    labels = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    sc = None if scale is None else torch.tensor([scale], device=dev)
    ops.label_rows(view, torch.tensor(t, device=dev) if with_targets else None, pad, sc, with_targets, loss,
                   lp if logprobs else None, amax, torch.tensor(mask, device=dev), MASKED, labels)
    torch.cuda.synchronize()
    guard = torch.ones_like(big, dtype=torch.bool)
    guard[r0:r0 + rows, c0:c0 + k] = False
    assert bool(torch.isnan(big[guard]).all()), "a guard element of the logits buffer was written"
    guard = torch.ones_like(lp_big, dtype=torch.bool)
    guard[r0:, c0:c0 + k] = False
    assert bool(torch.isnan(lp_big[guard]).all()), "a guard element of the log-probability buffer was written"
    return {"loss": loss.cpu().numpy(), "grad": view.cpu().numpy(), "logprobs": lp.cpu().numpy(),
            "argmax": amax.cpu().numpy(), "labels": labels.cpu().numpy()}


def _check(name, exp, got):
    x, t, mask, pad = make_case(name)
    for key in ("loss", "grad", "logprobs"):
        err = _err(got[key], exp[key])
        print("{} {}: error {:.3g} (unit {:.3g}, bound {:.3g})".format(name, key, err, exp["unit_" + key],
                                                                       exp["bound_" + key]))
        assert err <= exp["bound_" + key], (name, key, err, exp["bound_" + key])
    assert np.array_equal(got["argmax"], exp["argmax"]), name
    assert np.array_equal(got["labels"], exp["labels"]), name
    where = special_rows(len(t))
    assert got["argmax"][where["equal"]] == 0                                    # ties: the first maximum
    assert got["loss"][where["pad"]] == 0.0 and not got["grad"][where["pad"]].any()      # exact zeros
    assert got["labels"][where["masked"]] == MASKED               # the encoder's mask picks the label ...
    if CASES[name][2] > 1:
        assert got["loss"][where["masked"]] > 0.0                   # ... the loss is masked by the TARGETS alone
    assert (got["labels"][mask == 0] == MASKED).all() and np.array_equal(got["labels"][mask != 0],
                                                                         got["argmax"][mask != 0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_loss_gradient_argmax_and_logprobs_in_one_call(dev, name):
    from neuralmonkey_amd import ops
    assert ops.label_rows_max_classes() == 1024           # (3, 1028) is the fallback, (5, 1024) the packed kernel
    exp = expectations(name)
    got = _run(dev, name)
    _check(name, exp, got)
    again = _run(dev, name)                               # two runs are bit-equal (no floating-point atomics)
    for key in got:
        assert np.array_equal(got[key], again[key], equal_nan=True), (name, key)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["k43_ld48", "k65", "k1028_fallback"])
def test_strided_slice_of_a_nan_buffer_and_a_device_grad_scale(dev, name):
    """Logits and log-probabilities are interior slices (row and column offsets) of NaN-filled buffers whose guard
    elements stay NaN; ``grad_scale`` is a device scalar."""
    scale = 0.37
    got = _run(dev, name, scale=scale, offset=(1, 3))
    _check(name, expectations(name, scale), got)
    plain = _run(dev, name)
    assert np.array_equal(got["loss"], plain["loss"]) and np.array_equal(got["logprobs"], plain["logprobs"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["k43_ld48", "k1028_fallback"])
def test_inference_without_targets(dev, name):
    """targets = NULL: no loss, no gradient -- the logits are untouched, the loss buffer is not written."""
    x, _, _, _ = make_case(name)
    exp = expectations(name)
    got = _run(dev, name, with_targets=False)
    assert np.array_equal(got["grad"], x) and np.isnan(got["loss"]).all()
    assert _err(got["logprobs"], exp["logprobs"]) <= exp["bound_logprobs"]
    assert np.array_equal(got["argmax"], exp["argmax"]) and np.array_equal(got["labels"], exp["labels"])
    bare = _run(dev, name, with_targets=False, logprobs=False)
    assert np.array_equal(bare["argmax"], exp["argmax"]) and np.isnan(bare["logprobs"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [43, 1028])
def test_batch_of_pad_targets_only(dev, k):
    from neuralmonkey_amd import ops
    rng = np.random.default_rng(k)
    x = torch.tensor(rng.standard_normal((6, k)).astype(np.float32), device=dev)
    t = torch.zeros(6, dtype=torch.int32, device=dev)
    loss = torch.full((6,), float("nan"), device=dev)
    ops.label_rows(x, t, 0, None, True, loss)
    total = ops.reduce_sum(loss, torch.full((1,), float("nan"), device=dev))
    torch.cuda.synchronize()
    assert not loss.cpu().numpy().any() and not x.cpu().numpy().any() and float(total.cpu()[0]) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("k", [43, 1028])
def test_out_of_range_target_gives_nan_loss_and_zero_gradient(dev, k):
    from neuralmonkey_amd import ops
    rng = np.random.default_rng(k + 1)
    x = rng.standard_normal((4, k)).astype(np.float32)
    t = np.array([k, 3, -5, 0], np.int32)                 # too large, fine, negative, <pad>
    xd = torch.tensor(x, device=dev)
    loss = torch.full((4,), 7.0, device=dev)
    ops.label_rows(xd, torch.tensor(t, device=dev), 0, None, True, loss)
    torch.cuda.synchronize()
    got, grad = loss.cpu().numpy(), xd.cpu().numpy()
    assert np.isnan(got[[0, 2]]).all() and got[3] == 0.0 and not grad[[0, 2, 3]].any()
    want = R.rows(x[1:2], t[1:2], 0)
    assert abs(got[1] - want["loss"][0]) <= 1e-4 * abs(want["loss"][0])
    assert np.abs(grad[1] - want["grad"][0]).max() <= 1e-3 * np.abs(want["grad"]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [43, 1028])
def test_overlapping_logprobs_are_refused_on_both_paths(dev, k):
    """The same range test above and below the packed kernel's class bound: a log-probability buffer that starts
    inside the logits is refused before anything is launched."""
    from neuralmonkey_amd import _lib, ops
    buf = torch.zeros(8 * k, device=dev)
    logits = buf[:4 * k].view(4, k)
    for start in (0, 8, 3 * k):
        with pytest.raises(_lib.NMHipError, match="logprobs aliasing logits"):
            ops.label_rows(logits, logprobs=buf[start:start + 4 * k].view(4, k))
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any()


@pytest.mark.gpu
def test_autodiff_op_overwrites_the_logits_with_their_gradient(dev):
    """autodiff.label_xent on a recording tape: the logits become grad_scale * d sum(loss) / d logits; on a tape that
    does not record they stay, and argmax / labels come from the same call."""
    from neuralmonkey_amd import autodiff as F
    name = "k43_ld48"
    x, t, mask, pad = make_case(name)
    exp = expectations(name, 0.5)

    class Ctx:                                            # what a Tape asks of a run context (no session: no arena)
        device = None
        bufs = {}

        def buffer(self, key, shape, dtype=torch.float32, zero=False, zero_init=False):
            return self.bufs.setdefault((key, tuple(shape), dtype), torch.zeros(tuple(shape), dtype=dtype, device=dev))

    tape = F.Tape(Ctx(), "label_test", recording=True)
    var = tape.leaf(torch.tensor(x, device=dev), needs_grad=True)
    loss = F.label_xent(tape, var, torch.tensor(t, device=dev), pad, torch.tensor([0.5], device=dev))
    torch.cuda.synchronize()
    assert var.grad is var.data
    assert _err(loss.cpu().numpy(), exp["loss"]) <= exp["bound_loss"]
    assert _err(var.grad.cpu().numpy(), exp["grad"]) <= exp["bound_grad"]
    tape = F.Tape(Ctx(), "label_test_run", recording=False)
    var = tape.leaf(torch.tensor(x, device=dev), needs_grad=True)
    amax = torch.empty(len(t), dtype=torch.int32, device=dev)
    labels = torch.empty(len(t), dtype=torch.int32, device=dev)
    F.label_xent(tape, var, None, pad, None, None, amax, torch.tensor(mask, device=dev), MASKED, labels)
    torch.cuda.synchronize()
    assert var.grad is None and np.array_equal(var.data.cpu().numpy(), x)
    assert np.array_equal(amax.cpu().numpy(), exp["argmax"]) and np.array_equal(labels.cpu().numpy(), exp["labels"])


# each entry point of include/nmhip_label.h -> the test above that calls it (the rules of
# tests/test_pointwise_refs.py::ledger_problems; checked in tests/test_labeler_host.py)
LEDGER = {
    "nm_label_rows_max_classes": HERE + "test_loss_gradient_argmax_and_logprobs_in_one_call via ops.label_rows_max_classes",
    "nm_label_rows": HERE + "test_loss_gradient_argmax_and_logprobs_in_one_call via ops.label_rows",
    "nm_label_rows_from_stats": HERE + "test_loss_gradient_argmax_and_logprobs_in_one_call via ops.label_rows",
}
