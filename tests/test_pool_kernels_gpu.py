"""The kernels of the sentence-level heads (csrc/nm_pool.hip) called through ``ops`` on the MI355X against
tests/pool_ref.py.

Pooling cases (``POOL_CASES``): T = 1, and T = 7 with the lengths 7, 1, 3, 0, 7 in one batch, at D = 1, 5 (scalar path),
64 (16-byte path), 260 (two workgroups per sentence) -- the states a slice of a NaN-filled buffer with ldx > D, once at a
16-byte aligned column offset (vector path) and once at an odd one (scalar path).  Every case holds a column that is
negative at every real position, in a full-length sentence (pools to its true maximum) and in a padded one (pools to
1e-15, every padded position ties, no gradient), and two real positions holding the identical maximum (half the
gradient each).  ``accumulate`` runs on and off.

Softmax cases (``SOFTMAX_CASES``): the same T and lengths at H = 1, 5, 17 and 70 (two workgroups per sentence), the
energies of one sentence shifted by +100 and of another by -110 (without the maximum subtracted their exponentials
overflow / all underflow in float32), with the mask and without.

Tolerances: max pooling is a selection -- forward, ties and backward (one division where ties > 1, one addition with
``accumulate``) must EQUAL the float32 evaluation of the restatement.  An accumulating call is restated as prior +
gradient in both precisions, so its unit contains the rounding of the addition.  Average, softmax and squared error use the
project's unit method (tests/test_label_kernels_gpu.py): the UNIT is the error of the float32 NumPy evaluation of the
restatement against its float64 evaluation on the case's own inputs, never below one float32 epsilon of the largest
magnitude; the kernel is allowed ``MULTIPLE`` = 16 units, never more than smoke()'s caps (1e-4 of the largest magnitude
on a forward value, 1e-3 on a gradient)."""
import numpy as np
import pytest
import torch

from . import pool_ref as R

MULTIPLE = 16.0
EPS32 = float(np.finfo(np.float32).eps)
pytestmark = pytest.mark.gpu

LENGTHS7 = [7, 1, 3, 0, 7]
# name -> (seed, T, lengths, D, ldx, column offset of the slice in its NaN-filled buffer)
POOL_CASES = {
    "t1_d5": (1, 1, [1, 1, 0], 5, 5, 0),
    "t7_d1": (2, 7, LENGTHS7, 1, 1, 0),
    "t7_d5_ld9": (3, 7, LENGTHS7, 5, 9, 2),
    "t7_d64": (4, 7, LENGTHS7, 64, 64, 0),
    "t7_d260_ld272_vec": (5, 7, LENGTHS7, 260, 272, 4),
    "t7_d260_ld272_odd": (6, 7, LENGTHS7, 260, 272, 1),
    "t9_d8": (7, 9, [9, 2, 5, 0, 9], 8, 8, 0),
}
# name -> (seed, T, lengths, H, lde)
SOFTMAX_CASES = {
    "t1_h5": (11, 1, [1, 1, 0], 5, 5),
    "t7_h1": (12, 7, LENGTHS7, 1, 1),
    "t7_h5_ld8": (13, 7, LENGTHS7, 5, 8),
    "t7_h17": (14, 7, LENGTHS7, 17, 17),
    "t7_h70": (15, 7, LENGTHS7, 70, 70),
    "t300_h3": (16, 300, [300, 1, 150, 0, 299], 3, 3),
}


def mask_of(lengths, steps):
    return (np.arange(steps)[None, :] < np.asarray(lengths)[:, None]).astype(np.float32)


def make_pool_case(name):
    """(x [B, T, D] float32, mask [B, T] float32, dout [B, D] float32)."""
    seed, steps, lengths, d, _, _ = POOL_CASES[name]
    rng = np.random.default_rng(seed)
    bsz = len(lengths)
    x = (1.5 * rng.standard_normal((bsz, steps, d))).astype(np.float32)
    mask = mask_of(lengths, steps)
    dout = rng.standard_normal((bsz, d)).astype(np.float32)
    if steps >= 7:
        x[bsz - 1, :, d - 1] = -np.abs(x[bsz - 1, :, d - 1]) - 0.5        # negative everywhere, no padding
        x[2, :, d - 1] = -np.abs(x[2, :, d - 1]) - 0.5                    # negative everywhere, 4 padded positions
        x[0, 2, 0] = x[0, 5, 0] = 7.25                                    # the identical maximum at two real positions
        if d > 1:
            x[2, 0, 0] = x[2, 2, 0] = 6.5
    return x, mask, dout


def strided(dev, arr, ld, offset):
    """``arr`` [B, T, D] as a slice of a NaN-filled [B, T, ld + offset + 3] ... buffer with row stride ld'."""
    bsz, steps, d = arr.shape
    big = torch.full((bsz, steps, max(ld, d + offset)), float("nan"), device=dev)
    view = big[:, :, offset:offset + d]
    view.copy_(torch.tensor(arr, device=dev))
    return big, view


def bound(got32, want64, cap):
    mag = float(np.abs(want64).max()) if want64.size else 0.0
    unit = max(float(np.abs(np.asarray(got32, np.float64) - want64).max()) if want64.size else 0.0, EPS32 * mag)
    return min(MULTIPLE * unit, cap * mag), unit


def run_pool(dev, name, mode, accumulate=False):
    from neuralmonkey_amd import ops
    x, mask, dout = make_pool_case(name)
    _, steps, lengths, d, ld, off = POOL_CASES[name]
    bsz = len(lengths)
    big, view = strided(dev, x, ld + off if off else ld, off)
    m = torch.tensor(mask, device=dev)
    out = torch.full((bsz, d), float("nan"), device=dev)
    ties = torch.full((bsz, d), -7, dtype=torch.int32, device=dev) if mode == "max" else None
    ops.pool_fwd(mode, view, m, out, ties)
    rng = np.random.default_rng(99)
    prior = rng.standard_normal(x.shape).astype(np.float32)
    dbig, dview = strided(dev, prior if accumulate else np.full_like(x, np.nan), ld + off if off else ld, off)
    ops.pool_bwd(mode, torch.tensor(dout, device=dev), m, dview, x=view if mode == "max" else None,
                 out=out if mode == "max" else None, ties=ties, accumulate=accumulate)
    torch.cuda.synchronize()
    outside = torch.ones_like(big, dtype=torch.bool)
    outside[:, :, off:off + d] = False
    assert bool(torch.isnan(big[outside]).all()) and bool(torch.isnan(dbig[outside]).all()), "wrote outside its slice"
    return (out.cpu().numpy(), None if ties is None else ties.cpu().numpy(), dview.cpu().numpy(), prior)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("name", list(POOL_CASES))
def test_max_pooling_equals_the_float32_restatement(dev, name, accumulate):
    x, mask, dout = make_pool_case(name)
    out, ties, dx, prior = run_pool(dev, name, "max", accumulate)
    f32 = R.max_pool(x, mask, np.float32)
    assert np.array_equal(out, f32["out"]) and out.dtype == np.float32
    assert np.array_equal(ties, f32["ties"])
    want = R.max_pool_bwd(x, mask, dout, np.float32)
    if accumulate:
        want = (prior + want).astype(np.float32)
    assert np.array_equal(dx, want)
    lengths = POOL_CASES[name][2]
    steps, d = x.shape[1], x.shape[2]
    if steps >= 7:                                                 # the properties the case was built for
        last = len(lengths) - 1
        assert out[last, d - 1] < 0 and ties[last, d - 1] == 1
        assert out[2, d - 1] == np.float32(1e-15) and ties[2, d - 1] == steps - lengths[2]
        assert out[3].tolist() == [np.float32(1e-15)] * d and (ties[3] == steps).all()      # the empty sentence
        assert ties[0, 0] == 2 and out[0, 0] == np.float32(7.25)
        if not accumulate:
            assert dx[0, 2, 0] == dx[0, 5, 0] == np.float32(dout[0, 0] / np.float32(2)) and dx[0, 3, 0] == 0
            assert not dx[2, :, d - 1].any() and not dx[3].any()
    if not accumulate:                                             # exact zeros at every padded position
        assert not dx[mask == 0].any()


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("name", list(POOL_CASES))
def test_average_pooling_within_the_unit_bound(dev, name, accumulate):
    x, mask, dout = make_pool_case(name)
    out, _, dx, prior = run_pool(dev, name, "avg", accumulate)
    want = R.avg_pool(x, mask)["out"]
    tol, unit = bound(R.avg_pool(x, mask, np.float32)["out"], want, 1e-4)
    err = float(np.abs(out - want).max())
    print("avg fwd {}: err {:.3e} unit {:.3e} bound {:.3e}".format(name, err, unit, tol))
    assert err <= tol
    empty = [b for b, n in enumerate(POOL_CASES[name][2]) if n == 0]
    assert not out[empty].any()                                    # a sentence of length 0: exact zeros
    d = x.shape[2]
    want_dx = R.avg_pool_bwd(mask, dout, d)
    f32_dx = R.avg_pool_bwd(mask, dout, d, np.float32)
    if accumulate:                    # the restatement of an accumulating call is prior + gradient, in both precisions
        want_dx, f32_dx = prior.astype(np.float64) + want_dx, (prior + f32_dx).astype(np.float32)
    tol, unit = bound(f32_dx, want_dx, 1e-3)
    err = float(np.abs(dx.astype(np.float64) - want_dx).max())
    print("avg bwd {}: err {:.3e} unit {:.3e} bound {:.3e}".format(name, err, unit, tol))
    assert err <= tol
    if not accumulate:
        assert not dx[mask == 0].any()


def make_softmax_case(name):
    seed, steps, lengths, h, _ = SOFTMAX_CASES[name]
    rng = np.random.default_rng(seed)
    bsz = len(lengths)
    e = (2.0 * rng.standard_normal((bsz, steps, h))).astype(np.float32)
    e[0] += np.float32(100.0)
    e[2] -= np.float32(110.0)
    dw = rng.standard_normal((bsz, steps, h)).astype(np.float32)
    return e, mask_of(lengths, steps), dw


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("name", list(SOFTMAX_CASES))
def test_time_softmax_forward_and_backward_within_the_unit_bound(dev, name, masked):
    from neuralmonkey_amd import ops
    e, mask, dw = make_softmax_case(name)
    _, steps, lengths, h, lde = SOFTMAX_CASES[name]
    bsz = len(lengths)
    mk = mask if masked else None
    big, view = strided(dev, e, lde, 0)
    m = torch.tensor(mask, device=dev) if masked else None
    w = torch.full((bsz, steps, h), float("nan"), device=dev)
    s = torch.full((bsz, steps, h), float("nan"), device=dev)
    z = torch.full((bsz, h), float("nan"), device=dev)
    ops.time_softmax_fwd(view, m, w, s, z)
    f64, f32 = R.time_softmax(e, mk), R.time_softmax(e, mk, np.float32)
    for key, got in (("w", w), ("s", s)):
        tol, unit = bound(f32[key], f64[key], 1e-4)
        err = float(np.abs(got.cpu().numpy() - f64[key]).max())
        print("softmax {} {} masked={}: err {:.3e} unit {:.3e} bound {:.3e}".format(key, name, masked, err, unit, tol))
        assert err <= tol, key
    if masked:
        empty = [b for b, n in enumerate(lengths) if n == 0]
        assert not w[empty].cpu().numpy().any()
        assert not w.cpu().numpy()[mask == 0].any()
        # (a sentence's weights sum to 1 only as far as the 1e-8 of the denominator is small beside its real
        # positions' share of the plain softmax: the restatement's sums are the expectation)
        assert np.allclose(w.cpu().numpy().sum(axis=1), f64["w"].sum(axis=1), atol=1e-5)
    # backward, from the kernel's own s and Z; once overwriting, once accumulating
    want = R.time_softmax_bwd(dw, f64["s"], f64["z"], mk)
    tol, unit = bound(R.time_softmax_bwd(dw, f32["s"], f32["z"], mk, np.float32), want, 1e-3)
    dwt = torch.tensor(dw, device=dev)
    de = torch.full((bsz, steps, h), float("nan"), device=dev)
    ops.time_softmax_bwd(dwt, s, z if masked else None, m, de)
    err = float(np.abs(de.cpu().numpy() - want).max())
    print("softmax bwd {} masked={}: err {:.3e} unit {:.3e} bound {:.3e}".format(name, masked, err, unit, tol))
    assert err <= tol
    prior = np.random.default_rng(5).standard_normal(e.shape).astype(np.float32)
    acc = torch.tensor(prior, device=dev)
    ops.time_softmax_bwd(dwt, s, z if masked else None, m, acc, accumulate=True)
    f32_acc = (prior + R.time_softmax_bwd(dw, f32["s"], f32["z"], mk, np.float32)).astype(np.float32)
    tol_acc, unit_acc = bound(f32_acc, prior.astype(np.float64) + want, 1e-3)     # prior + gradient, restated in float32
    err = float(np.abs(acc.cpu().numpy().astype(np.float64) - (prior.astype(np.float64) + want)).max())
    print("softmax bwd accumulating {} masked={}: err {:.3e} unit {:.3e} bound {:.3e}".format(name, masked, err, unit_acc,
                                                                                           tol_acc))
    assert err <= tol_acc
    assert bool(torch.isnan(big[:, :, h:]).all())
    # in place: w over e
    ops.time_softmax_fwd(view, m, view)
    assert np.array_equal(view.cpu().numpy(), w.cpu().numpy())


@pytest.mark.parametrize("rows,dim,ld", [(1, 1, 1), (5, 2, 2), (300, 5, 7), (7, 1, 3)])
def test_squared_error_rows_within_the_unit_bound(dev, rows, dim, ld):
    from neuralmonkey_amd import ops
    rng = np.random.default_rng(rows * 10 + dim)
    p = (3.0 * rng.standard_normal((rows, dim))).astype(np.float32)
    y = (3.0 * rng.standard_normal(rows)).astype(np.float32)
    scale = 0.37
    big = torch.full((rows, ld), float("nan"), device=dev)
    view = big[:, :dim]
    view.copy_(torch.tensor(p, device=dev))
    loss = torch.full((rows,), float("nan"), device=dev)
    ops.sqerr_rows(view, torch.tensor(y, device=dev), None, False, loss)              # the loss alone: p untouched
    assert np.array_equal(view.cpu().numpy(), p)
    f64, f32 = R.sqerr(p, y, scale), R.sqerr(p, y, scale, np.float32)
    tol, unit = bound(f32["loss"], f64["loss"], 1e-4)
    err = float(np.abs(loss.cpu().numpy() - f64["loss"]).max())
    print("sqerr loss: err {:.3e} unit {:.3e} bound {:.3e}".format(err, unit, tol))
    assert err <= tol
    ops.sqerr_rows(view, torch.tensor(y, device=dev), torch.tensor([scale], device=dev), True, None)
    tol, unit = bound(f32["grad"], f64["grad"], 1e-3)
    err = float(np.abs(view.cpu().numpy() - f64["grad"]).max())
    print("sqerr grad: err {:.3e} unit {:.3e} bound {:.3e}".format(err, unit, tol))
    assert err <= tol
    assert bool(torch.isnan(big[:, dim:]).all())


def test_two_runs_are_bit_equal(dev):
    from neuralmonkey_amd import ops
    rng = np.random.default_rng(3)
    x = torch.tensor(rng.standard_normal((6, 50, 260)).astype(np.float32), device=dev)
    mask = torch.tensor(mask_of([50, 1, 17, 0, 33, 50], 50), device=dev)
    outs = []
    for _ in range(2):
        out = torch.empty((6, 260), device=dev)
        ops.pool_fwd("avg", x, mask, out)
        e = x[:, :, :8].contiguous()
        w = torch.empty_like(e)
        ops.time_softmax_fwd(e, mask, w)
        outs.append((out.cpu().numpy(), w.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
