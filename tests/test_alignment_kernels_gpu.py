"""The supervised-attention kernels (csrc/nm_align.hip) called through ``ops.align_xent`` / ``ops.align_softmax`` on the
MI355X against tests/align_ref.py in float64.

Shapes (T, B, S) (``SHAPES``): one row of one position; a few ragged rows; tests/alignment.ini's own (8, 16, 12); both sides
of the lane count (64 | 65); 257; and 1500, many trips per lane.  The weights are random in [0, 1] with row sums of at
most 1 and exact zeros (padded source positions); the fed array is [B, T + 2, S + 3] with NaN in everything the rows
must not read, so both strides matter and a read past T or S poisons an output; rows cycle through a normalised label
row, an all-zero one, one that does not sum to 1 and a padded position (tests/align_ref.py:random_case).

Modes: ``accumulate`` 0 and 1 (onto a random gradient), ``dw=None``, ``scale`` NULL and a device scalar; every output
lies between guard floats that must stay as they were; two runs of one launch are bit-equal.

Tolerances, the convention of tests/test_label_kernels_gpu.py: the UNIT is the error of the float32 NumPy evaluation of
the restatement against its float64 evaluation on the case's own inputs, never below one float32 epsilon of the largest
magnitude; the kernel is allowed 16 units, never more than 1e-4 relative on the loss, 1e-3 of the largest magnitude on
the gradient and 1e-4 of the largest magnitude (that file's log-probability cap) on ``align_softmax``."""
import numpy as np
import pytest
import torch

from . import align_ref as R

pytestmark = pytest.mark.gpu

MULTIPLE = 16.0
EPS32 = float(np.finfo(np.float32).eps)
GUARD = 8
SHAPES = [(1, 1, 1), (3, 2, 5), (8, 16, 12), (5, 3, 64), (4, 3, 65), (2, 2, 257), (2, 1, 1500)]
CAPS = {"loss_rows": 1e-4, "grad": 1e-3, "decoded": 1e-4}
_CASES = {}


def base_gradient(shape):
    """What ``dw`` holds before an accumulating launch (the product's gradient in the model)."""
    return np.random.default_rng(5).standard_normal(shape).astype(np.float32)


def case(shape):
    """The inputs of a shape and its float64 expectations with their bounds, computed once."""
    if shape not in _CASES:
        rng = np.random.default_rng(1000 + sum(shape))
        w, target, pad = R.random_case(rng, *shape)
        exp = {}
        base = base_gradient(shape)
        for scale in (1.0, 0.37):
            r64, r32 = R.rows(w, target, pad, scale, np.float64), R.rows(w, target, pad, scale, np.float32)
            r64["grad+base"], r32["grad+base"] = r64["grad"] + base, r32["grad"] + base      # ``accumulate``
            for key, cap in list(CAPS.items()) + [("grad+base", CAPS["grad"])]:
                mag = float(np.abs(r64[key]).max())
                unit = max(float(np.abs(r32[key].astype(np.float64) - r64[key]).max()), EPS32 * mag)
                exp[(key, scale)] = (r64[key], min(MULTIPLE * unit, cap * mag))
        _CASES[shape] = (w, target, pad, exp)
    return _CASES[shape]


def guarded(dev, shape, fill=None):
    """A device tensor of ``shape`` between GUARD floats of -7.5 on either side (full buffer, view)."""
    n = int(np.prod(shape))
    full = torch.full((n + 2 * GUARD,), -7.5, dtype=torch.float32, device=dev)
    view = full[GUARD:GUARD + n].view(*shape)
    if fill is not None:
        view.copy_(torch.as_tensor(fill))
    return full, view


def guards_intact(full):
    host = full.cpu().numpy()
    return bool((host[:GUARD] == -7.5).all() and (host[-GUARD:] == -7.5).all())


def check(got, want_bound, what):
    want, bound = want_bound
    got = np.asarray(got.cpu().numpy(), np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what + ": something of the NaN tail reached an output"
    err = float(np.abs(got - want).max())
    print("{}: max |diff| {:.3e}, bound {:.3e}".format(what, err, bound))
    assert err <= bound, "{}: max |diff| {:.3e} above {:.3e}".format(what, err, bound)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_align_xent_against_float64(dev, shape):
    from neuralmonkey_amd import ops
    w, target, pad, exp = case(shape)
    steps, bsz, slen = shape
    wd, td, pd = (torch.as_tensor(a).to(dev) for a in (w, target, pad))
    scale_d = torch.tensor([0.37], dtype=torch.float32, device=dev)
    base = base_gradient(shape)
    # loss alone
    lfull, loss = guarded(dev, (steps, bsz))
    ops.align_xent(wd, td, pd, loss)
    check(loss, exp[("loss_rows", 1.0)], "loss rows, dw=None")
    assert guards_intact(lfull)
    assert not loss.cpu().numpy()[pad == 0].any()                    # exact zeros
    total = torch.empty(1, dtype=torch.float32, device=dev)
    ops.reduce_sum(loss.reshape(-1), total)
    want = float(exp[("loss_rows", 1.0)][0].sum())
    assert abs(float(total[0]) - want) <= 1e-4 * abs(want) + 1e-7
    for scale, scale_t in ((1.0, None), (0.37, scale_d)):
        for accumulate in (False, True):
            lfull, loss = guarded(dev, (steps, bsz))
            dfull, dw = guarded(dev, shape, fill=base)
            ops.align_xent(wd, td, pd, loss, scale=scale_t, dw=dw, accumulate=accumulate)
            what = "scale {} accumulate {}".format(scale, int(accumulate))
            check(loss, exp[("loss_rows", 1.0)], what + " loss rows")
            check(dw, exp[("grad+base" if accumulate else "grad", scale)], what + " gradient")
            assert guards_intact(lfull) and guards_intact(dfull)
            got = dw.cpu().numpy()
            if accumulate:
                assert np.array_equal(got[pad == 0], base[pad == 0])           # nothing added
            else:
                assert not got[pad == 0].any()
            # the same launch again: bit-equal
            lfull2, loss2 = guarded(dev, (steps, bsz))
            dfull2, dw2 = guarded(dev, shape, fill=base)
            ops.align_xent(wd, td, pd, loss2, scale=scale_t, dw=dw2, accumulate=accumulate)
            assert torch.equal(lfull, lfull2) and torch.equal(dfull, dfull2)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_align_softmax_against_float64(dev, shape):
    from neuralmonkey_amd import ops
    w, _, _, exp = case(shape)
    steps, bsz, slen = shape
    wd = torch.as_tensor(w).to(dev)
    full, out = guarded(dev, (bsz, steps, slen))
    ops.align_softmax(wd, out)
    check(out, exp[("decoded", 1.0)], "softmax")
    assert guards_intact(full)
    full2, out2 = guarded(dev, (bsz, steps, slen))
    ops.align_softmax(wd, out2)
    assert torch.equal(full, full2)


def test_one_step_of_a_larger_target(dev):
    """The taped path's launch: step t alone, the fed array entered at row t through a view."""
    from neuralmonkey_amd import ops
    shape = (3, 2, 5)
    w, target, pad, exp = case(shape)
    wd, td, pd = (torch.as_tensor(a).to(dev) for a in (w, target, pad))
    loss = torch.zeros(3, 2, dtype=torch.float32, device=dev)
    dw = torch.zeros(shape, dtype=torch.float32, device=dev)
    for t in range(3):
        ops.align_xent(wd[t:t + 1], td[:, t:], pd[t:t + 1], loss[t:t + 1], dw=dw[t:t + 1], accumulate=True)
    check(loss, exp[("loss_rows", 1.0)], "loss rows, step by step")
    check(dw, exp[("grad", 1.0)], "gradient, step by step")


def test_wrapper_refuses_what_does_not_fit(dev):
    from neuralmonkey_amd import ops
    w = torch.zeros(3, 2, 5, device=dev)
    pad, loss = torch.ones(3, 2, device=dev), torch.zeros(3, 2, device=dev)
    for bad in ((2, 2, 5), (3, 3, 5), (2, 3, 4)):
        with pytest.raises(AssertionError):
            ops.align_xent(w, torch.zeros(bad, device=dev), pad, loss)
    with pytest.raises(AssertionError):
        ops.align_softmax(w, torch.zeros(3, 2, 5, device=dev))           # [B, T, S] is wanted
    empty = torch.zeros(0, 2, 5, device=dev)
    ops.align_xent(empty, torch.zeros(2, 4, 5, device=dev), torch.zeros(0, 2, device=dev),
                   torch.zeros(0, 2, device=dev))                          # T*B == 0: a no-op
