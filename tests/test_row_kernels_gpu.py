"""The vocabulary-row kernels of csrc/nm_logits.hip -- nm_row_stats (row_scan_kernel<4, 8 | 16 | 32, false> and the
scalar row_stats_kernel), nm_xent (xent_regs_kernel<8 | 16>, xent_kernel), nm_xent_colsum (xent_cols_kernel<2 | 4 | 8>)
and nm_gumbel_argmax -- against the float64 references of tests/row_cases.py on its case table: every dispatch branch,
both sides of every boundary, strided and misaligned views in buffers padded with 3e38, maxima and targets in every
float4 lane, ties across threads, lanes and waves, -inf classes, logits near +-1e4, targets outside [0, V), signed row
weights, every combination of the optional arguments.  tests/test_row_cases_ref.py shows on the CPU that the table
covers the dispatch rules and where the bounds C_* come from (the float32 numpy restatement, not these kernels)."""
import itertools

import numpy as np
import pytest
import torch

from . import row_cases as RC

pytestmark = pytest.mark.gpu


def _up(a, dev, dtype=None):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype).to(dev)


def _dview(flat_t, rows, lay):
    return torch.as_strided(flat_t, (rows, lay.v), (lay.ldx, 1), lay.off)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _stats_outputs(dev, rows):
    return (torch.full((rows,), float("nan"), device=dev), torch.full((rows,), float("nan"), device=dev),
            torch.full((rows,), -7, dtype=torch.int32, device=dev))


# ------------------------------------------------------------------------------------------------------------------
# row statistics
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in RC.STATS_CASES])
def test_row_statistics_against_float64(dev, name):
    from neuralmonkey_amd import ops
    b = RC.build_stats(name)
    rows = len(b.kinds)
    x = _dview(_up(b.flat, dev), rows, b.lay)
    assert (x.data_ptr() % 16 == 0) == b.lay.aligned
    mx, lse, am = _stats_outputs(dev, rows)
    ops.row_stats(x, mx, lse, am)
    mx, lse, am = mx.cpu().numpy(), lse.cpu().numpy(), am.cpu().numpy()
    err = RC.scaled(lse, b.lse)
    print(name, RC.row_scan_nv(b.lay.v, b.lay.ldx, b.lay.aligned), "lse error {:.3e} (C_LSE {:.1e})".format(err, RC.C_LSE))
    assert np.array_equal(_bits(mx), _bits(b.max)), (b.kinds, mx, b.max)
    assert np.array_equal(am, b.argmax), (b.kinds, am, b.argmax)
    for r, want in b.pinned.items():
        assert am[r] == want, b.kinds[r]
    assert err <= RC.C_LSE


@pytest.mark.parametrize("name", RC.SUBSET_CASES)
def test_row_statistics_every_subset_of_the_outputs(dev, name):
    from neuralmonkey_amd import ops
    b = RC.build_stats(name)
    rows = len(b.kinds)
    x = _dview(_up(b.flat, dev), rows, b.lay)
    full = _stats_outputs(dev, rows)
    ops.row_stats(x, *full)
    assert np.array_equal(full[2].cpu().numpy(), b.argmax) and RC.scaled(full[1].cpu().numpy(), b.lse) <= RC.C_LSE
    for asked in itertools.product((False, True), repeat=3):
        outs = _stats_outputs(dev, rows)
        ops.row_stats(x, *[o if on else None for o, on in zip(outs, asked)])
        for o, want, on in zip(outs, full, asked):
            if on:
                assert torch.equal(o, want), asked
    torch.cuda.synchronize()


def test_row_statistics_of_no_rows_writes_nothing(dev):
    from neuralmonkey_amd import _lib
    x = torch.zeros(4, 64, device=dev)
    mx, lse, am = _stats_outputs(dev, 4)
    code = _lib.load().nm_row_stats(torch.cuda.current_stream().cuda_stream, x.data_ptr(), 64, 0, 64, mx.data_ptr(),
                                    lse.data_ptr(), am.data_ptr())
    _lib.check(code, "nm_row_stats")
    torch.cuda.synchronize()
    assert torch.isnan(mx).all() and torch.isnan(lse).all() and (am == -7).all()


@pytest.mark.parametrize("v,variant", RC.DEGENERATE_LAYOUTS)
def test_degenerate_rows_still_yield_a_valid_argmax(dev, v, variant):
    """A row with no element above -inf (all -inf, or all NaN after a diverged step) gives the first index, not the
    0x7fffffff the running index starts from: nm_greedy_update hands the value on as a symbol."""
    from neuralmonkey_amd import ops
    x_np, want = RC.degenerate_rows(v)
    x = _up(x_np, dev)
    mx, lse, am = _stats_outputs(dev, 4)
    ops.row_stats(x, mx, lse, am)
    am = am.cpu().numpy()
    print(v, "argmax of [ordinary, all -inf, all NaN, NaN in every other column]:", am, "want", want)
    assert ((am >= 0) & (am < v)).all(), am
    for r in (0, 1, 3):
        assert am[r] == want[r], (r, am)
    ref_max, _, ref_lse = RC.ref_stats(x_np[:1])
    assert mx.cpu().numpy()[0] == ref_max[0] and RC.scaled(lse.cpu().numpy()[:1], ref_lse) <= RC.C_LSE
    only = torch.full((4,), -7, dtype=torch.int32, device=dev)          # the scalar kernel without its exp pass
    ops.row_stats(x, None, None, only)
    assert np.array_equal(only.cpu().numpy(), am)


# ------------------------------------------------------------------------------------------------------------------
# cross entropy
# ------------------------------------------------------------------------------------------------------------------
def _check_gradient(got, ref, unit, bound, what):
    err = RC.in_units(got, ref, unit)
    print(what, "error {:.3e} of the unit (bound {:.1e})".format(err, bound))
    assert err <= bound, what


@pytest.mark.parametrize("name", [c.name for c in RC.XENT_CASES])
def test_cross_entropy_against_float64(dev, name):
    from neuralmonkey_amd import ops
    b = RC.build_xent(name)
    c = b.case
    pad = RC.padding(b.rows, b.lay)
    tgt, w, gs = _up(b.targets, dev), _up(b.weights, dev), _up(None if b.grad_scale is None else [b.grad_scale], dev)
    want_loss = c.options[2]

    def call(write_grad, with_loss):
        flat = _up(b.flat, dev)
        loss = torch.full((b.rows,), float("nan"), device=dev) if with_loss else None
        ops.xent(_dview(flat, b.rows, b.lay), tgt, w, loss, gs, write_grad, c.eps)
        return flat.cpu().numpy(), None if loss is None else loss.cpu().numpy()

    branch = RC.xent_nv(b.lay.v, b.lay.ldx, b.lay.aligned)
    flat0, loss0 = call(False, want_loss)
    assert np.array_equal(_bits(flat0), _bits(b.flat))               # no gradient asked: nothing written
    flat1, loss1 = call(True, want_loss)
    if want_loss:
        err = RC.scaled(loss1, b.ref.loss)
        print(name, branch, "loss error {:.3e} (bound {:.1e})".format(err, RC.loss_bound(b)))
        assert np.isfinite(loss1).all(), loss1
        assert err <= RC.loss_bound(b)
        assert np.array_equal(_bits(loss0), _bits(loss1))
    assert np.array_equal(_bits(flat1[pad]), _bits(b.flat[pad]))     # the padding comes back bit-identical
    _check_gradient(RC.view(flat1, b.rows, b.lay), b.ref.grad, b.ref.unit, RC.C_G, name + " " + branch + " gradient")
    flat2, _ = call(True, not want_loss)                             # with / without loss_rows: the same gradient
    assert np.array_equal(_bits(flat2), _bits(flat1))


# ------------------------------------------------------------------------------------------------------------------
# cross entropy with column sums
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in RC.COLS_CASES])
def test_cross_entropy_with_column_sums_against_float64(dev, name):
    from neuralmonkey_amd import ops
    b = RC.build_cols(name)
    c = b.case
    pad = RC.padding(b.rows, b.lay)
    tgt, w, gs = _up(b.targets, dev), _up(b.weights, dev), _up([b.grad_scale], dev)
    flat, flat_x = _up(b.flat, dev), _up(b.flat, dev)
    loss, loss_x = torch.full((b.rows,), float("nan"), device=dev), torch.full((b.rows,), float("nan"), device=dev)
    partial = torch.full((c.g, c.v), float("nan"), device=dev)
    assert ops.xent_colsum_ok(_dview(flat, b.rows, b.lay))
    ops.xent_colsum(_dview(flat, b.rows, b.lay), tgt, w, loss, gs, c.eps, partial)
    ops.xent(_dview(flat_x, b.rows, b.lay), tgt, w, loss_x, gs, True, c.eps)
    bias = torch.full((c.v,), float("nan"), device=dev)
    ops.colsum(partial, bias)
    got, got_loss, got_part, got_bias = flat.cpu().numpy(), loss.cpu().numpy(), partial.cpu().numpy(), bias.cpu().numpy()
    branch = RC.colsum_nv(b.lay.v, b.lay.ldx, b.lay.aligned, True, b.rows, c.g)
    err = RC.scaled(got_loss, b.ref.loss)
    print(name, branch, "loss error {:.3e} (bound {:.1e})".format(err, RC.C_LOSS))
    assert np.isfinite(got_loss).all() and err <= RC.C_LOSS
    assert np.array_equal(_bits(got[pad]), _bits(b.flat[pad]))
    _check_gradient(RC.view(got, b.rows, b.lay), b.ref.grad, b.ref.unit, RC.C_G, name + " gradient")
    assert np.array_equal(_bits(got), _bits(flat_x.cpu().numpy()))   # bit-equal to nm_xent, loss and gradient
    assert np.array_equal(_bits(got_loss), _bits(loss_x.cpu().numpy()))
    ref_part, unit_part, ref_bias, unit_bias = RC.ref_colsum(b.ref, c.g)
    assert not np.isnan(got_part).any()
    _check_gradient(got_part, ref_part, unit_part, RC.C_P, name + " partials")
    _check_gradient(got_bias, ref_bias, unit_bias, RC.C_B, name + " bias gradient")


@pytest.mark.parametrize("what,v,extra,off,poff,rows,g", RC.COLS_REFUSALS, ids=[r[0] for r in RC.COLS_REFUSALS])
def test_column_sum_refusals_leave_everything_untouched(dev, what, v, extra, off, poff, rows, g):
    from neuralmonkey_amd import _lib
    lay = RC.Layout(v, v + extra, off)
    assert RC.colsum_nv(v, lay.ldx, lay.aligned, poff % 4 == 0, rows, g).startswith("refuse:")
    flat_np = RC.new_buffer(rows, lay)
    RC.view(flat_np, rows, lay)[:] = 0.25
    flat = _up(flat_np, dev)
    partial = torch.full((max(g, 1) * v + 4,), float("nan"), device=dev)
    tgt, loss = torch.zeros(rows, dtype=torch.int32, device=dev), torch.full((rows,), float("nan"), device=dev)
    code = _lib.load().nm_xent_colsum(torch.cuda.current_stream().cuda_stream, flat.data_ptr() + 4 * off, lay.ldx, rows,
                                      v, tgt.data_ptr(), None, loss.data_ptr(), None, 0.0, partial.data_ptr() + 4 * poff,
                                      g)
    assert code != 0
    with pytest.raises(_lib.NMHipError, match="nm_xent_colsum"):
        _lib.check(code, "nm_xent_colsum")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(flat.cpu().numpy()), _bits(flat_np))
    assert torch.isnan(partial).all() and torch.isnan(loss).all()


# ------------------------------------------------------------------------------------------------------------------
# the draw
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in RC.DRAW_CASES])
def test_draw_equals_the_restated_gumbel_argmax(dev, name):
    """The rule of tests/test_sampling_gpu.py on strided rows padded with 3e38: within 1e-4 of the restated maximum,
    exact in at least 95 % of the rows (the CPU test shows that the table's seeds allow every row)."""
    from neuralmonkey_amd import ops
    c = RC.DRAW_BY_NAME[name]
    lay, flat, x_np = RC.build_draw(name)
    x = _dview(_up(flat, dev), c.rows, lay)
    for salt in RC.DRAW_SALTS:
        out = torch.full((c.rows,), -7, dtype=torch.int32, device=dev)
        ops.gumbel_argmax(x, salt, out)
        got = out.cpu().numpy()
        assert ((got >= 0) & (got < c.v)).all(), got          # never the padding
        want, noisy = RC.f32_draw(x_np, salt)
        gap = noisy[np.arange(c.rows), want] - noisy[np.arange(c.rows), got]
        assert (gap <= RC.DRAW_GAP).all(), gap.max()
        assert (got == want).mean() >= 0.95
        if c.v == 1:
            assert (got == 0).all()
