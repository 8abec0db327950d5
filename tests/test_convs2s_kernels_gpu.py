"""The residual layer of the convolutional sequence-to-sequence encoder on the MI355X (include/nmhip_convs2s.h): the
fused conv1d + GLU + residual kernels (MFMA and scalar) and their gradients against float64 torch restatements, and the
taped functions built on them (autodiff.conv1d_glu, add_position_param, time_max) against float64 autograd.

Tolerances are built the way tests/test_sentence_cnn_gpu.py builds them: 1e-6 times the same expression evaluated on
the absolute values of the operands (sigmoid bounded by 1, sigmoid' by 1/4) plus 1e-7, times 10.  The test of the
weight gradient's slab path uses the derived summation bound of tests/conv1d_ref.py instead."""
import math

import pytest
import torch

from . import conv1d_ref as R
from .conv1d_ref import _pre, _ref_conv_t, _ref_wgrad

pytestmark = pytest.mark.gpu


def _tol(scale):
    return 10 * (1e-6 * scale + 1e-7)


def _within(got, want, scale, what):
    err = (got.double().cpu() - want).abs()
    assert bool((err <= _tol(scale)).all()), "{}: {:.3e} over a bound of {:.3e}".format(
        what, float(err.max()), float(_tol(scale).flatten()[int(err.argmax())]))


def _padded(shape, pad, dev, fill=7.0):
    """A [B, T, C] view with row stride C + pad of a buffer filled with ``fill``."""
    full = torch.full(shape[:2] + (shape[2] + pad,), fill, device=dev)
    return full, full[:, :, :shape[2]]


CASES = [  # (B, T, C, w, algo, (pad of ldx, ldy, lddy, lddx))
    (3, 7, 10, 5, 0, (0, 0, 0, 0)),          # tests/bpe.ini's layer
    (2, 1, 10, 5, 0, (0, 0, 0, 0)),          # one position: every tap but the centre in padding
    (2, 3, 13, 8, 0, (0, 0, 0, 0)),          # T < w, the widest MFMA width
    (2, 9, 13, 2, 0, (0, 0, 0, 0)),          # pad 0 before, 1 after
    (2, 30, 64, 1, 0, (0, 0, 0, 0)),         # width 1
    (1, 129, 40, 3, 0, (0, 0, 0, 0)),        # two position tiles with a halo across the seam, C no tile multiple
    (2, 131, 200, 5, 0, (0, 0, 0, 0)),       # several feature tiles, a channel-chunk remainder, partners far apart
    (2, 23, 13, 9, 0, (0, 0, 0, 0)),         # auto falls back to the scalar path
    (2, 29, 40, 4, 2, (0, 0, 0, 0)),         # scalar path forced
    (2, 37, 13, 5, 0, (3, 5, 2, 7)),         # ldx, ldy, lddy, lddx > C
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B{}-T{}-C{}-w{}-algo{}{}".format(
    c[0], c[1], c[2], c[3], c[4], "-strided" if any(c[5]) else ""))
def test_glu_layer_forward_and_gradients_match_float64(dev, case):
    from neuralmonkey_amd import ops
    bsz, steps, c, width, algo, (px, py, pdy, pdx) = case
    g = torch.Generator().manual_seed(11)
    x = torch.randn(bsz, steps, c, generator=g, dtype=torch.float64)
    w = torch.randn(width, c, 2 * c, generator=g, dtype=torch.float64) * math.sqrt(4.0 / c) / math.sqrt(width)
    b = torch.randn(2 * c, generator=g, dtype=torch.float64) * 0.3
    dy = torch.randn(bsz, steps, c, generator=g, dtype=torch.float64)
    f32 = lambda t: t.float().contiguous().to(dev)
    x_full, xd = _padded((bsz, steps, c), px, dev)
    xd.copy_(x.float())
    dy_full, dyd = _padded((bsz, steps, c), pdy, dev)
    dyd.copy_(dy.float())
    wd, bd = f32(w), f32(b)
    x, w, b, dy = xd.double().cpu(), wd.double().cpu(), bd.double().cpu(), dyd.double().cpu()   # the rounded operands

    # ---- forward: with the save buffers, and without; y bit-equal -------------------------------------------------
    y_full, y = _padded((bsz, steps, c), py, dev)
    y2_full, y2 = _padded((bsz, steps, c), py, dev)
    lin = torch.full((bsz * steps, c), float("nan"), device=dev)
    sig = torch.full((bsz * steps, c), float("nan"), device=dev)
    ops.conv1d_glu_fwd(xd, wd, bd, y, lin, sig, algo=algo)
    ops.conv1d_glu_fwd(xd, wd, bd, y2, algo=algo)
    torch.cuda.synchronize()
    assert torch.equal(y_full, y2_full)                                      # (and the pad columns: both untouched)
    if py:
        assert bool((y_full[:, :, c:] == 7.0).all())
    x64 = x.clone().requires_grad_(True)
    w64 = w.clone().requires_grad_(True)
    b64 = b.clone().requires_grad_(True)
    z = _pre(x64, w64, b64)
    ref_lin, ref_sig = z[..., :c], torch.sigmoid(z[..., c:])
    ref = ref_lin * ref_sig + x64
    z_abs = _pre(x.abs(), w.abs(), b.abs())
    _within(y, ref.detach(), z_abs[..., :c] + x.abs(), "y")
    _within(lin.view(bsz, steps, c), ref_lin.detach(), z_abs[..., :c], "lin_save")
    _within(sig.view(bsz, steps, c), ref_sig.detach(), 0.25 * z_abs[..., c:], "sig_save")

    # ---- backward: onto non-zero buffers ---------------------------------------------------------------------------
    ref.backward(dy)
    ref_dz = torch.cat([dy * ref_sig, dy * ref_lin * ref_sig * (1 - ref_sig)], -1).detach()
    s_dz = torch.cat([dy.abs(), dy.abs() * z_abs[..., :c] * 0.25], -1)
    s_dx = dy.abs() + _ref_conv_t(s_dz, [w.abs()], [(width, 2 * c)])
    s_dw = _ref_wgrad(x.abs(), s_dz, width)
    s_db = s_dz.sum((0, 1))
    wsp = torch.empty(max(1, ops.conv1d_glu_workspace_floats(bsz, steps, c, width)), device=dev)

    def run(accumulate):
        dz = torch.full((bsz * steps, 2 * c), float("nan"), device=dev)
        start = (0.5, 0.125, 0.25) if accumulate else (float("nan"),) * 3
        dx_full, dx = _padded((bsz, steps, c), pdx, dev)
        dx.fill_(start[0])
        dw = torch.full_like(wd, start[1])
        db = torch.full_like(bd, start[2])
        ops.conv1d_glu_bwd(xd, wd, lin, sig, dyd, dz, dx=dx, accumulate_dx=accumulate, dfilt=dw, dbias=db,
                           accumulate_params=accumulate, workspace=wsp, algo=algo)
        torch.cuda.synchronize()
        return dz, dx_full, dx, dw, db
    dz, dx_full, dx, dw, db = run(True)
    _within(dz.view(bsz, steps, 2 * c), ref_dz, s_dz, "dz")
    _within(dx - 0.5, x64.grad, s_dx, "dx (accumulated)")
    _within(dw - 0.125, w64.grad, s_dw, "dW (accumulated)")
    _within(db - 0.25, b64.grad, s_db, "dbias (accumulated)")
    if pdx:
        assert bool((dx_full[:, :, c:] == 7.0).all())
    # ... a second run is bit-equal
    dz2, dx2_full, _, dw2, db2 = run(True)
    assert torch.equal(dz, dz2) and torch.equal(dx_full, dx2_full) and torch.equal(dw, dw2) and torch.equal(db, db2)
    # ... and without the accumulate flags whatever the buffers held is overwritten
    _, _, dx3, dw3, db3 = run(False)
    _within(dx3, x64.grad, s_dx, "dx")
    _within(dw3, w64.grad, s_dw, "dW")
    _within(db3, b64.grad, s_db, "dbias")
    # ... dx alone: no parameter gradient, no workspace
    dz4 = torch.empty(bsz * steps, 2 * c, device=dev)
    dx4_full, dx4 = _padded((bsz, steps, c), pdx, dev)
    ops.conv1d_glu_bwd(xd, wd, lin, sig, dyd, dz4, dx=dx4, algo=algo)
    torch.cuda.synchronize()
    assert torch.equal(dx4, dx3)


SLAB_RUNS = [("G1", (0, 0, 0, 0)), ("G1", (3, 5, 2, 7)), ("G2", (0, 0, 0, 0)), ("G3", (0, 0, 0, 0))]


@pytest.mark.parametrize("name,pads", SLAB_RUNS, ids=lambda v: v if isinstance(v, str) else (
    "strided" if any(v) else "dense"))
def test_glu_gradients_over_several_slabs_meet_the_fp32_sum_bound(dev, name, pads):
    """G1-G3 of tests/conv1d_ref.py: the weight gradient in two to four position slabs (G2, G3: slab seams on sentence
    seams, where the halo taps read zero and not the neighbouring sentence).  The gradient sums are compared with
    float64 sums of the device's own dz (read back once it has passed the dz check of the test above), under the
    summation bounds of tests/conv1d_ref.py; the workspace holds NaN before every call."""
    from neuralmonkey_amd import ops
    (bsz, steps, c, width), _, slices, per, last = R.GLU_SLAB_CASES[name]
    px, py, pdy, pdx = pads
    plan = R.slab_plan(bsz, steps, c, R.glu_filters(c, width))
    assert (plan["slices"], plan["per"], plan["last"]) == (slices, per, last)
    assert ops.conv1d_glu_workspace_floats(bsz, steps, c, width) * 4 == plan["bytes"]
    g = torch.Generator().manual_seed(13 + int(name[1:]))
    x = torch.randn(bsz, steps, c, generator=g, dtype=torch.float64)
    w = torch.randn(width, c, 2 * c, generator=g, dtype=torch.float64) * math.sqrt(4.0 / c) / math.sqrt(width)
    b = torch.randn(2 * c, generator=g, dtype=torch.float64) * 0.3
    dy = torch.randn(bsz, steps, c, generator=g, dtype=torch.float64)
    f32 = lambda t: t.float().contiguous().to(dev)
    x_full, xd = _padded((bsz, steps, c), px, dev)
    xd.copy_(x.float())
    dy_full, dyd = _padded((bsz, steps, c), pdy, dev)
    dyd.copy_(dy.float())
    wd, bd = f32(w), f32(b)
    x, w, b, dy = xd.double().cpu(), wd.double().cpu(), bd.double().cpu(), dyd.double().cpu()   # the rounded operands

    y_full, y = _padded((bsz, steps, c), py, dev)
    lin = torch.full((bsz * steps, c), float("nan"), device=dev)
    sig = torch.full((bsz * steps, c), float("nan"), device=dev)
    ops.conv1d_glu_fwd(xd, wd, bd, y, lin, sig, algo=0)
    torch.cuda.synchronize()
    z = _pre(x, w, b)
    ref_lin, ref_sig = z[..., :c], torch.sigmoid(z[..., c:])
    z_abs = _pre(x.abs(), w.abs(), b.abs())
    _within(y, ref_lin * ref_sig + x, z_abs[..., :c] + x.abs(), "y")
    _within(lin.view(bsz, steps, c), ref_lin, z_abs[..., :c], "lin_save")
    _within(sig.view(bsz, steps, c), ref_sig, 0.25 * z_abs[..., c:], "sig_save")
    ref_dz = torch.cat([dy * ref_sig, dy * ref_lin * ref_sig * (1 - ref_sig)], -1)
    s_dz = torch.cat([dy.abs(), dy.abs() * z_abs[..., :c] * 0.25], -1)

    def run(accumulate, algo):
        dz = torch.full((bsz * steps, 2 * c), float("nan"), device=dev)
        start = (0.5, 0.125, 0.25) if accumulate else (float("nan"),) * 3
        dx_full, dx = _padded((bsz, steps, c), pdx, dev)
        dx.fill_(start[0])
        dw = torch.full_like(wd, start[1])
        db = torch.full_like(bd, start[2])
        wsp = torch.full((plan["bytes"] // 4,), float("nan"), device=dev)
        ops.conv1d_glu_bwd(xd, wd, lin, sig, dyd, dz, dx=dx, accumulate_dx=accumulate, dfilt=dw, dbias=db,
                           accumulate_params=accumulate, workspace=wsp, algo=algo)
        torch.cuda.synchronize()
        return dz, dx_full, dx, dw, db
    first = run(False, 0)
    _within(first[0].view(bsz, steps, 2 * c), ref_dz, s_dz, "dz")
    dz = first[0].double().cpu().view(bsz, steps, 2 * c)                  # the operand of every gradient sum
    assert all(bool((t > 0).any()) and bool((t < 0).any()) for t in (dz, x, w, dy))
    filters = R.glu_filters(c, width)
    want = (dy + _ref_conv_t(dz, [w], filters), _ref_wgrad(x, dz, width), dz.sum((0, 1)))
    mags = (dy.abs() + _ref_conv_t(dz.abs(), [w.abs()], filters), _ref_wgrad(x.abs(), dz.abs(), width),
            dz.abs().sum((0, 1)))
    ks = (width * 2 * c + 1, bsz * steps + slices, bsz * steps + 16)    # (dx: every tap and filter, and the residual dy)

    def check(out, accumulate, algo):
        tag = "" if algo == 0 else " (scalar)"
        label = "{}{} algo {} acc {}".format(name, " strided" if any(pads) else "", algo, int(accumulate))
        assert torch.equal(out[0], first[0])                               # one dz kernel, the same saves
        starts = (0.5, 0.125, 0.25) if accumulate else (0.0, 0.0, 0.0)
        for got, ref, mag, k, start, what in zip(out[2:], want, mags, ks, starts, ("dx", "dW", "dbias")):
            R.within(got, ref + start, k + int(accumulate), mag + start, label + " " + what, "glu " + what + tag)
        if pdx:
            assert bool((out[1][:, :, c:] == 7.0).all())
    check(first, False, 0)
    accumulated = run(True, 0)
    check(accumulated, True, 0)
    again = run(True, 0)
    assert all(torch.equal(p, q) for p, q in zip(accumulated, again))
    for accumulate in (False, True):
        check(run(accumulate, 2), accumulate, 2)
    for full, pad in ((x_full, px), (dy_full, pdy), (y_full, py)):
        assert not pad or bool((full[:, :, c:] == 7.0).all())


def test_forced_mfma_equals_auto_and_scalar_agrees(dev):
    """algo 1 is what auto takes for w <= 8 (bit-equal); the scalar kernel computes the same layer."""
    from neuralmonkey_amd import ops
    g = torch.Generator().manual_seed(5)
    bsz, steps, c, width = 2, 70, 48, 3
    x = torch.randn(bsz, steps, c, generator=g).to(dev)
    w = (torch.randn(width, c, 2 * c, generator=g) * math.sqrt(4.0 / c / width)).to(dev)
    b = (torch.randn(2 * c, generator=g) * 0.3).to(dev)
    ys = [torch.empty_like(x) for _ in range(3)]
    for algo, y in enumerate(ys):
        ops.conv1d_glu_fwd(x, w, b, y, algo=algo)
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[1])
    z_abs = _pre(x.double().cpu().abs(), w.double().cpu().abs(), b.double().cpu().abs())
    _within(ys[2], ys[1].double().cpu(), z_abs[..., :c] + x.double().cpu().abs(), "scalar against MFMA")


class _Ctx:                       # the tape needs buffers only
    def __init__(self, dev):
        self.device = dev
        self.session = type("Session", (), {})()

    def buffer(self, key, shape, dtype=torch.float32, zero=False):
        return torch.zeros(shape, dtype=dtype, device=self.device)


def test_taped_encoder_functions_match_float64_autograd(dev):
    """add_position_param -> conv1d_glu x 2 -> time_max on a tape: values and every gradient; the table's rows beyond T
    keep an exactly zero gradient; a tie over time splits the gradient evenly."""
    from neuralmonkey_amd import autodiff as F
    g = torch.Generator().manual_seed(9)
    bsz, steps, c, width, max_len = 3, 6, 12, 4, 9
    x = torch.randn(bsz, steps, c, generator=g, dtype=torch.float64)
    table = torch.randn(max_len, c, generator=g, dtype=torch.float64)
    ws = [torch.randn(width, c, 2 * c, generator=g, dtype=torch.float64) * math.sqrt(4.0 / c / width) for _ in range(2)]
    bs = [torch.randn(2 * c, generator=g, dtype=torch.float64) * 0.3 for _ in range(2)]
    d_out = torch.randn(bsz, c, generator=g, dtype=torch.float64)
    d_states = torch.randn(bsz, steps, c, generator=g, dtype=torch.float64)
    f32 = lambda t: t.float().contiguous().to(dev)
    tape = F.Tape(_Ctx(dev), "convs2s", recording=True)
    v = lambda t: F.Var(f32(t), torch.zeros_like(f32(t)), True)
    xv = F.Var(f32(x).view(bsz * steps, c), None, True)
    xv.is_leaf = True
    tv, wv, bv = v(table), [v(w) for w in ws], [v(b) for b in bs]
    h = F.add_position_param(tape, xv, tv, bsz, steps)
    for w, b in zip(wv, bv):
        h = F.conv1d_glu(tape, h, w, b, bsz, steps)
    out = F.time_max(tape, h, bsz, steps)
    F.ops.ew("copy", f32(d_states).view(bsz * steps, c), None, tape.grad(h), accumulate=True)
    F.ops.ew("copy", f32(d_out), None, tape.grad(out), accumulate=True)
    tape.backward()
    torch.cuda.synchronize()

    p = [t.clone().requires_grad_(True) for t in [x, table] + ws + bs]
    r = p[0] + p[1][:steps]
    for w, b in zip(p[2:4], p[4:6]):
        z = _pre(r, w, b)
        r = z[..., :c] * torch.sigmoid(z[..., c:]) + r
    ref_out = torch.amax(r, dim=1)
    (ref_out * d_out).sum().backward(retain_graph=True)
    (r * d_states).sum().backward()
    assert float((h.data.double().cpu().view(bsz, steps, c) - r.detach()).abs().max()) < 1e-5 * float(r.detach().abs().max())
    assert torch.equal(out.data.cpu(), h.data.view(bsz, steps, c).amax(dim=1).cpu())       # max_t x exactly
    for got, want, name in [(xv.grad.view(bsz, steps, c), p[0].grad, "x"), (tv.grad, p[1].grad, "table")] + [
            (a.grad, q.grad, "w") for a, q in zip(wv, p[2:4])] + [(a.grad, q.grad, "b") for a, q in zip(bv, p[4:6])]:
        err = (got.double().cpu() - want).abs().max() / (want.abs().max() + 1e-12)
        assert float(err) < 1e-5, (name, float(err))
    assert bool((tv.grad[steps:] == 0).all()) and bool((tv.grad[:steps] != 0).any())

    # a tie: two positions hold the maximum of one column; each takes half
    tape = F.Tape(_Ctx(dev), "ties", recording=True)
    xt = torch.randn(2, 5, 8, generator=g)
    xt[0, 1, 3] = xt[0, 4, 3] = 9.0
    hv = F.Var(f32(xt).view(10, 8), None, True)
    out = F.time_max(tape, hv, 2, 5)
    grad = torch.randn(2, 8, generator=g)
    F.ops.ew("copy", f32(grad), None, tape.grad(out), accumulate=True)
    tape.backward()
    torch.cuda.synchronize()
    got = hv.grad.view(2, 5, 8).cpu()
    assert got[0, 1, 3] == got[0, 4, 3] == grad[0, 3] / 2 and float(got[0, :, 3].abs().sum()) == abs(float(grad[0, 3]))
    x64 = xt.double().requires_grad_(True)
    (torch.amax(x64, dim=1) * grad.double()).sum().backward()
    assert torch.equal(got.double(), x64.grad.float().double())


# entry point of include/nmhip_convs2s.h -> the tests of this file that call it
ENTRY_POINTS = {
    "nm_conv1d_glu_fwd": ["test_glu_layer_forward_and_gradients_match_float64",
                          "test_glu_gradients_over_several_slabs_meet_the_fp32_sum_bound",
                          "test_forced_mfma_equals_auto_and_scalar_agrees",
                          "test_taped_encoder_functions_match_float64_autograd"],
    "nm_conv1d_glu_workspace_bytes": ["test_glu_layer_forward_and_gradients_match_float64",
                                      "test_glu_gradients_over_several_slabs_meet_the_fp32_sum_bound",
                                      "test_taped_encoder_functions_match_float64_autograd"],
    "nm_conv1d_glu_bwd": ["test_glu_layer_forward_and_gradients_match_float64",
                          "test_glu_gradients_over_several_slabs_meet_the_fp32_sum_bound",
                          "test_taped_encoder_functions_match_float64_autograd"],
}


def test_every_entry_point_has_a_test(dev):
    from neuralmonkey_amd import _lib
    assert set(ENTRY_POINTS) == set(_lib.CONVS2S_SIGNATURES)
    assert all(callable(globals()[name]) for names in ENTRY_POINTS.values() for name in names)
