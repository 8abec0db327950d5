"""Batch norm with statistics over several ranks' rows on the MI355X (include/nmhip_bnsync.h), in one process: the rows of
an array are cut into three unequal parts -- one of them a single row -- that play the ranks.  Each part's statistics
(nm_bn2d_part_stats) are merged (nm_bn2d_merge) and every part is normalised with the merged statistics (nm_bn2d_fwd in
inference mode); each part's channel sums (nm_bn2d_bwd_sums) are added up as the exchange between the ranks adds them
and every part's input gradient comes from the total (nm_bn2d_bwd_dx).  The references are float64 torch on the WHOLE
array; operands and bounds are those of tests/test_image_kernels_gpu.py for nm_bn2d_fwd / nm_bn2d_bwd.  With ONE part
everything is bit-equal to nm_bn2d_fwd / nm_bn2d_bwd."""
import pytest
import torch
import torch.nn.functional as TF

from . import cnn2d_models as M
from .test_image_kernels_gpu import BN_SHAPES, NAN, _bn_operands, _padded, _untouched, _within

pytestmark = pytest.mark.gpu

CUTS = {30: (17, 12, 1), 4290: (3000, 1289, 1)}
SHAPE_IDS = ["{}x{}".format(*s) for s in BN_SHAPES]


def _spans(rows, whole=False):
    sizes = (rows,) if whole else CUTS[rows]
    assert sum(sizes) == rows
    spans, lo = [], 0
    for n in sizes:
        spans.append((lo, lo + n))
        lo += n
    return spans


def _merged(ops, xd, spans, dev, moving=None):
    """-> (parts [world, 2C + 1], mean, var, total) of the row spans of xd, every output buffer NaN before."""
    c = xd.shape[1]
    parts = torch.full((len(spans), ops.bn2d_part_doubles(c)), NAN, device=dev, dtype=torch.float64)
    for r, (lo, hi) in enumerate(spans):
        ops.bn2d_part_stats(xd[lo:hi], parts[r])
    mean, var = torch.full((c,), NAN, device=dev), torch.full((c,), NAN, device=dev)
    total = torch.full((1,), NAN, device=dev, dtype=torch.float64)
    mm, mv = moving if moving is not None else (None, None)
    ops.bn2d_merge(parts, mean, var, total, moving_mean=mm, moving_var=mv)
    return parts, mean, var, total


def _normalised(ops, xd, spans, gamma, beta, mean, var, relu, dev):
    y_full, y = _padded(tuple(xd.shape), 2, dev)
    for lo, hi in spans:
        ops.bn2d_fwd(xd[lo:hi], gamma, beta, y[lo:hi], False, relu, moving_mean=mean, moving_var=var)
    return y_full, y


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=SHAPE_IDS)
def test_merged_statistics_and_output_match_float64_on_the_whole_array(dev, shape, relu):
    """The bounds are test_batch_norm_training_forward_and_moving_update's, on the whole array.  The channels at
    10 +- 0.1 are what a merge of sums of squares would fail."""
    from neuralmonkey_amd import ops
    rows, c = shape
    spans = _spans(rows)
    _, xd, gamma, beta = _bn_operands(rows, c, dev)
    x, g64, b64 = xd.double().cpu(), gamma.double().cpu(), beta.double().cpu()
    mm0, mv0 = torch.linspace(-1, 1, c), torch.linspace(0.5, 2, c)
    mm, mv = mm0.to(dev), mv0.to(dev)
    parts, mean, var, total = _merged(ops, xd, spans, dev, moving=(mm, mv))
    y_full, y = _normalised(ops, xd, spans, gamma, beta, mean, var, relu, dev)
    torch.cuda.synchronize()
    assert float(total) == rows and parts[:, 0].cpu().tolist() == [float(hi - lo) for lo, hi in spans]
    for r, (lo, hi) in enumerate(spans):                       # a part: the rounded mean, the deviations about it
        pm = parts[r, 1:1 + c].cpu()
        assert torch.equal(pm, pm.float().double())
        _within(pm, x[lo:hi].mean(0), x[lo:hi].abs().mean(0), "mean of part {}".format(r))
        m2 = ((x[lo:hi] - pm) ** 2).sum(0)
        _within(parts[r, 1 + c:], m2, m2 + 2 * (m2 * (hi - lo)).sqrt() * x[lo:hi].abs().mean(0), "M2 of part {}".format(r))
    assert not bool(parts[2, 1 + c:].any())                    # a single row deviates from itself by nothing
    ref_mean, ref_var = x.mean(0), x.var(0, unbiased=False)
    _within(mean, ref_mean, x.abs().mean(0), "batch mean")
    _within(var, ref_var, ref_var + 2 * ref_var.sqrt() * x.abs().mean(0), "batch variance")
    ref = TF.batch_norm(x, None, None, g64, b64, training=True, eps=M.EPSILON)
    ref = torch.relu(ref) if relu else ref
    rstd = 1.0 / torch.sqrt(ref_var + M.EPSILON)
    _within(y, ref, g64.abs() * (x.abs() + ref_mean.abs()) * rstd + b64.abs(), "y")
    assert _untouched(y_full, c)
    if relu:
        assert bool((y >= 0).all()) and bool((y == 0).any())
    # moving = 0.99 moving + 0.01 batch, the variance that goes in being the UNBIASED one over the GLOBAL count
    unbiased = ref_var * rows / (rows - 1)
    _within(mm, 0.99 * mm0.double() + 0.01 * ref_mean, 0.99 * mm0.double().abs() + 0.01 * ref_mean.abs(), "moving mean")
    _within(mv, 0.99 * mv0.double() + 0.01 * unbiased, 0.99 * mv0.double() + 0.01 * unbiased, "moving variance")
    if rows == 30:                                 # 30 / 29, not the 17 / 16 of the largest part
        assert float(((mv.double().cpu() - 0.99 * mv0.double()) / 0.01 / ref_var).mean()) == pytest.approx(
            rows / (rows - 1), rel=1e-2)
    # without the pointers nothing moves; a second run is bit-equal
    keep = (mm.clone(), mv.clone())
    parts2, mean2, var2, total2 = _merged(ops, xd, spans, dev)
    _, y2 = _normalised(ops, xd, spans, gamma, beta, mean2, var2, relu, dev)
    torch.cuda.synchronize()
    assert torch.equal(parts2, parts) and torch.equal(mean2, mean) and torch.equal(var2, var) and torch.equal(y2, y)
    assert torch.equal(total2, total) and torch.equal(mm, keep[0]) and torch.equal(mv, keep[1])


def _torch_grads(xd, gamma, beta, dyd, relu, dtype):
    p = [t.detach().cpu().to(dtype).requires_grad_(True) for t in (xd, gamma, beta)]
    out = TF.batch_norm(p[0], None, None, p[1], p[2], training=True, eps=M.EPSILON)
    out = torch.relu(out) if relu else out
    out.backward(dyd.cpu().to(dtype))
    return [t.grad.double() for t in p], out.detach()


def _gradients(ops, xd, y, dyd, gamma, mean, var, relu, spans, dev, accumulate):
    """The parts' sums, their total as the ranks' exchange forms it (added in rank order, float32), dx of every part
    from the total and the global row count; dgamma / dbeta collect the parts' own sums."""
    rows, c = xd.shape
    start = (0.5, 0.125, 0.25) if accumulate else (NAN,) * 3
    dx_full, dx = _padded((rows, c), 2, dev)
    dx.fill_(start[0])
    dg, db = torch.full((c,), start[1], device=dev), torch.full((c,), start[2], device=dev)
    sums = [torch.full((2 * c,), NAN, device=dev) for _ in spans]
    for r, (lo, hi) in enumerate(spans):
        ops.bn2d_bwd_sums(xd[lo:hi], y[lo:hi] if relu else None, dyd[lo:hi], mean, var, relu, sums[r], dgamma=dg, dbeta=db,
                          accumulate_params=accumulate or r > 0)
    total = sums[0].clone()
    for s in sums[1:]:
        total += s
    for lo, hi in spans:
        ops.bn2d_bwd_dx(xd[lo:hi], y[lo:hi] if relu else None, dyd[lo:hi], gamma, mean, var, relu, total, rows, dx[lo:hi],
                        accumulate_dx=accumulate)
    torch.cuda.synchronize()
    return dx_full, dx, dg, db, total


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=SHAPE_IDS)
def test_gradients_from_summed_sums_within_four_times_float32_torch(dev, shape, relu):
    """The bound of test_batch_norm_backward_within_four_times_float32_torch: four times the largest error of a float32
    torch evaluation on the CPU against float64 on the same inputs, per output, plus the 1e-7 floor; ReLU inputs within
    rounding of zero are left out of dx the same way."""
    from neuralmonkey_amd import ops
    rows, c = shape
    spans = _spans(rows)
    _, xd, gamma, beta = _bn_operands(rows, c, dev)
    g = torch.Generator().manual_seed(29)
    _, dyd = _padded((rows, c), 1, dev)
    dyd.copy_(torch.randn(rows, c, generator=g))
    _, mean, var, _ = _merged(ops, xd, spans, dev)
    _, y = _normalised(ops, xd, spans, gamma, beta, mean, var, relu, dev)
    want, out64 = _torch_grads(xd, gamma, beta, dyd, relu, torch.float64)
    single, _ = _torch_grads(xd, gamma, beta, dyd, relu, torch.float32)
    bounds = [4 * float((s - w).abs().max()) + 1e-7 for s, w in zip(single, want)]
    safe = torch.ones(rows, c, dtype=torch.bool) if not relu else (out64.abs() > 1e-5) | (out64 == 0) & (
        TF.batch_norm(xd.double().cpu(), None, None, gamma.double().cpu(), beta.double().cpu(), training=True,
                      eps=M.EPSILON) < -1e-5)
    dx_full, dx, dg, db, total = _gradients(ops, xd, y, dyd, gamma, mean, var, relu, spans, dev, False)
    for got, ref, bound, name in ((dx, want[0], bounds[0], "dx"), (dg, want[1], bounds[1], "dgamma"),
                                  (db, want[2], bounds[2], "dbeta")):
        err = (got.double().cpu() - ref).abs()
        if name == "dx":
            err = err[safe]
        print("bnsync bwd {}x{} relu={} {}: error {:.3e}, bound {:.3e}".format(rows, c, relu, name, float(err.max()), bound))
        assert float(err.max()) <= bound, "{}: {:.3e} over {:.3e}".format(name, float(err.max()), bound)
    # dgamma / dbeta hold the parts' own sums added up: the total of the exchange, formed in the same order
    assert _untouched(dx_full, c) and torch.equal(total[:c], db) and torch.equal(total[c:], dg)
    _, dx2, dg2, db2, _ = _gradients(ops, xd, y, dyd, gamma, mean, var, relu, spans, dev, False)
    assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2)           # bit-equal
    dx3_full, dx3, dg3, db3, _ = _gradients(ops, xd, y, dyd, gamma, mean, var, relu, spans, dev, True)
    assert _untouched(dx3_full, c)
    assert float((dx3 - 0.5 - dx).abs().max()) <= 1e-6 * (0.5 + float(dx.abs().max()))
    assert float((dg3 - 0.125 - dg).abs().max()) <= 1e-6 * (0.125 + float(dg.abs().max()))
    assert float((db3 - 0.25 - db).abs().max()) <= 1e-6 * (0.25 + float(db.abs().max()))


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=SHAPE_IDS)
def test_one_part_is_bit_equal_to_the_single_process_kernels(dev, shape, relu):
    """What makes a forced process group of one rank train exactly like no process group."""
    from neuralmonkey_amd import ops
    rows, c = shape
    spans = _spans(rows, whole=True)
    _, xd, gamma, beta = _bn_operands(rows, c, dev)
    g = torch.Generator().manual_seed(29)
    _, dyd = _padded((rows, c), 1, dev)
    dyd.copy_(torch.randn(rows, c, generator=g))
    mm0, mv0 = torch.linspace(-1, 1, c).to(dev), torch.linspace(0.5, 2, c).to(dev)
    # nm_bn2d_fwd (training) and nm_bn2d_bwd
    mm1, mv1 = mm0.clone(), mv0.clone()
    mean1, var1 = torch.full((c,), NAN, device=dev), torch.full((c,), NAN, device=dev)
    y1 = torch.full((rows, c), NAN, device=dev)
    ops.bn2d_fwd(xd, gamma, beta, y1, True, relu, moving_mean=mm1, moving_var=mv1, batch_mean=mean1, batch_var=var1)
    dx1, dg1, db1 = torch.full((rows, c), NAN, device=dev), torch.full((c,), NAN, device=dev), torch.full((c,), NAN, device=dev)
    sums1 = torch.full((2 * c,), NAN, device=dev)
    ops.bn2d_bwd(xd, y1 if relu else None, dyd, gamma, mean1, var1, relu, sums1, dx=dx1, dgamma=dg1, dbeta=db1,
                 accumulate_params=False)
    # the four entry points with one part
    mm2, mv2 = mm0.clone(), mv0.clone()
    _, mean2, var2, total = _merged(ops, xd, spans, dev, moving=(mm2, mv2))
    _, y2 = _normalised(ops, xd, spans, gamma, beta, mean2, var2, relu, dev)
    _, dx2, dg2, db2, sums2 = _gradients(ops, xd, y2, dyd, gamma, mean2, var2, relu, spans, dev, False)
    torch.cuda.synchronize()
    assert float(total) == rows
    for a, b, name in ((mean1, mean2, "batch mean"), (var1, var2, "batch variance"), (mm1, mm2, "moving mean"),
                       (mv1, mv2, "moving variance"), (y1, y2, "y"), (sums1, sums2, "sums"), (dx1, dx2, "dx"),
                       (dg1, dg2, "dgamma"), (db1, db2, "dbeta")):
        assert torch.equal(a, b), name
    assert not torch.equal(mm1, mm0) and not torch.equal(mv1, mv0)


# entry point of include/nmhip_bnsync.h -> the tests of this file that call it
ENTRY_POINTS = {
    "nm_bn2d_part_stats": ["test_merged_statistics_and_output_match_float64_on_the_whole_array",
                           "test_one_part_is_bit_equal_to_the_single_process_kernels"],
    "nm_bn2d_merge": ["test_merged_statistics_and_output_match_float64_on_the_whole_array",
                      "test_one_part_is_bit_equal_to_the_single_process_kernels"],
    "nm_bn2d_bwd_sums": ["test_gradients_from_summed_sums_within_four_times_float32_torch",
                         "test_one_part_is_bit_equal_to_the_single_process_kernels"],
    "nm_bn2d_bwd_dx": ["test_gradients_from_summed_sums_within_four_times_float32_torch",
                       "test_one_part_is_bit_equal_to_the_single_process_kernels"],
}


def test_every_entry_point_has_a_test(dev):
    from neuralmonkey_amd import _lib
    assert set(ENTRY_POINTS) == set(_lib.BNSYNC_SIGNATURES)
    assert all(name in globals() for tests in ENTRY_POINTS.values() for name in tests)
