"""The image stack on the MI355X (include/nmhip_image.h): the conv2d kernels (MFMA and scalar) and their gradients, the
batch norm, the pooling windows and the column transpose against float64 torch (functions on the CPU, autograd for the
gradients) and the NumPy restatement of tests/cnn2d_models.py, and the taped functions of image_ops against float64
autograd.

Operands live in padded buffers whose padding is NaN; outputs are written into NaN-filled buffers.  Tolerances are built
the way tests/test_convs2s_kernels_gpu.py builds them: 1e-6 times the same expression evaluated on the absolute values of
the operands plus 1e-7, times 10."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from . import cnn2d_models as M

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _tol(scale):
    return 10 * (1e-6 * scale + 1e-7)


def _within(got, want, scale, what):
    err = (got.double().cpu() - want).abs()
    bound = _tol(scale) + torch.zeros_like(err)
    assert bool((err <= bound).all()), "{}: {:.3e} over a bound of {:.3e}".format(
        what, float(err.max()), float(bound.flatten()[int(err.argmax())]))


def _padded(shape, pad, dev, dtype=torch.float32):
    """A view of ``shape`` whose rows lie shape[-1] + pad apart in a buffer of NaN."""
    full = torch.full(tuple(shape[:-1]) + (shape[-1] + pad,), NAN, device=dev, dtype=dtype)
    return full, full[..., :shape[-1]]


def _untouched(full, cols):
    return cols == full.shape[-1] or bool(torch.isnan(full[..., cols:]).all())


def _conv64(x, w, b, pad):
    """tf.layers.conv2d at stride 1 in float64: x [B, H, W, Cin], w [k, k, Cin, Cout]."""
    k = w.shape[0]
    xc = x.permute(0, 3, 1, 2)
    if pad == "same":
        before = (k - 1) // 2
        xc = TF.pad(xc, (before, k - 1 - before, before, k - 1 - before))
    return TF.conv2d(xc, w.permute(3, 2, 0, 1), b).permute(0, 2, 3, 1)


CONV_CASES = [  # (B, H, W, Cin, Cout, k, pad)
    (2, 5, 7, 1, 4, 3, "valid"),         # one input channel
    (3, 4, 6, 5, 12, 2, "same"),         # even k: nothing padded before, one row and column after
    (2, 6, 9, 17, 70, 3, "same"),        # channels off the 16-channel chunk, output columns across a 64-wide tile
    (1, 3, 140, 4, 4, 3, "valid"),       # a row longer than a 128-position tile
    (2, 7, 5, 12, 12, 1, "same"),        # 1 x 1
    (2, 9, 8, 3, 5, 5, "same"),          # k = 5: two padded rows on every side
]


@pytest.mark.parametrize("algo", [1, 2], ids=["mfma", "scalar"])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "B{}-{}x{}-{}to{}-k{}-{}".format(*c))
def test_conv2d_forward_and_gradients_match_float64(dev, case, algo):
    from neuralmonkey_amd import ops
    bsz, h, w, cin, cout, k, pad = case
    g = torch.Generator().manual_seed(13)
    oh, ow = ops.conv2d_out_hw(h, w, k, pad)
    x_full, xd = _padded((bsz, h, w, cin), 3, dev)
    xd.copy_(torch.randn(bsz, h, w, cin, generator=g))
    dy_full, dyd = _padded((bsz, oh, ow, cout), 2, dev)
    dyd.copy_(torch.randn(bsz, oh, ow, cout, generator=g))
    wd = (torch.randn(k, k, cin, cout, generator=g) / math.sqrt(k * k * cin)).to(dev)
    bd = (torch.randn(cout, generator=g) * 0.3).to(dev)
    x, wt, b, dy = xd.double().cpu(), wd.double().cpu(), bd.double().cpu(), dyd.double().cpu()      # the rounded operands

    y_full, y = _padded((bsz, oh, ow, cout), 5, dev)
    ops.conv2d_fwd(xd, wd, bd, y, pad, algo=algo)
    y2_full, y2 = _padded((bsz, oh, ow, cout), 5, dev)
    ops.conv2d_fwd(xd, wd, bd, y2, pad, algo=algo)
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and _untouched(y_full, cout)
    p = [t.clone().requires_grad_(True) for t in (x, wt, b)]
    ref = _conv64(*p, pad)
    a = [t.abs().clone().requires_grad_(True) for t in (x, wt, b)]
    ref_abs = _conv64(*a, pad)
    _within(y, ref.detach(), ref_abs.detach(), "y")
    assert np.abs(M.np_conv2d(x.numpy(), wt.numpy(), b.numpy(), pad) - ref.detach().numpy()).max() < 1e-12
    ref.backward(dy)
    ref_abs.backward(dy.abs())                                   # the same sums over absolute operands: the scales
    s_dx, s_dw, s_db = a[0].grad, a[1].grad, a[2].grad
    wsp = torch.empty(max(1, ops.conv2d_workspace_floats(bsz, h, w, cin, k, cout, pad)), device=dev)

    def run(accumulate):
        start = (0.5, 0.125, 0.25) if accumulate else (NAN,) * 3
        dx_full, dx = _padded((bsz, h, w, cin), 4, dev)
        dx.fill_(start[0])
        dw, db = torch.full_like(wd, start[1]), torch.full_like(bd, start[2])
        ops.conv2d_bwd(xd, wd, dyd, pad, dx=dx, accumulate_dx=accumulate, dfilt=dw, dbias=db,
                       accumulate_params=accumulate, workspace=wsp, algo=algo)
        torch.cuda.synchronize()
        return dx_full, dx, dw, db
    dx_full, dx, dw, db = run(True)
    _within(dx - 0.5, p[0].grad, s_dx, "dx (accumulated)")
    _within(dw - 0.125, p[1].grad, s_dw, "dW (accumulated)")
    _within(db - 0.25, p[2].grad, s_db, "dbias (accumulated)")
    assert _untouched(dx_full, cin)
    _, dx2, dw2, db2 = run(True)                                 # a second run is bit-equal
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    _, dx3, dw3, db3 = run(False)                                # without the flags the NaN is overwritten
    _within(dx3, p[0].grad, s_dx, "dx")
    _within(dw3, p[1].grad, s_dw, "dW")
    _within(db3, p[2].grad, s_db, "dbias")
    _, dx4 = _padded((bsz, h, w, cin), 4, dev)                   # dx alone: no workspace
    ops.conv2d_bwd(xd, wd, dyd, pad, dx=dx4, algo=algo)
    db5 = torch.full_like(bd, NAN)                               # parameters alone: no dx
    ops.conv2d_bwd(xd, wd, dyd, pad, dbias=db5, accumulate_params=False, workspace=wsp, algo=algo)
    torch.cuda.synchronize()
    assert torch.equal(dx4, dx3) and torch.equal(db5, db3)


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "B{}-{}x{}-{}to{}-k{}-{}".format(*c))
def test_conv2d_algos_agree_and_auto_is_one_of_them(dev, case):
    from neuralmonkey_amd import ops
    bsz, h, w, cin, cout, k, pad = case
    g = torch.Generator().manual_seed(17)
    oh, ow = ops.conv2d_out_hw(h, w, k, pad)
    x = torch.randn(bsz, h, w, cin, generator=g).to(dev)
    dy = torch.randn(bsz, oh, ow, cout, generator=g).to(dev)
    wd = (torch.randn(k, k, cin, cout, generator=g) / math.sqrt(k * k * cin)).to(dev)
    bd = (torch.randn(cout, generator=g) * 0.3).to(dev)
    wsp = torch.empty(max(1, ops.conv2d_workspace_floats(bsz, h, w, cin, k, cout, pad)), device=dev)
    outs = []
    for algo in (0, 1, 2):
        y = torch.full((bsz, oh, ow, cout), NAN, device=dev)
        dx, dw, db = torch.full_like(x, NAN), torch.full_like(wd, NAN), torch.full_like(bd, NAN)
        ops.conv2d_fwd(x, wd, bd, y, pad, algo=algo)
        ops.conv2d_bwd(x, wd, dy, pad, dx=dx, dfilt=dw, dbias=db, accumulate_params=False, workspace=wsp, algo=algo)
        outs.append((y, dx, dw, db))
    torch.cuda.synchronize()
    a = [t.double().cpu().abs().requires_grad_(True) for t in (x, wd, bd)]
    ref_abs = _conv64(*a, pad)
    ref_abs.backward(dy.double().cpu().abs())
    scales = (ref_abs.detach(), a[0].grad, a[1].grad, a[2].grad)
    for i, name in enumerate(("y", "dx", "dW", "dbias")):
        _within(outs[2][i], outs[1][i].double().cpu(), scales[i], "scalar against MFMA: " + name)
        assert torch.equal(outs[0][i], outs[1][i]) or torch.equal(outs[0][i], outs[2][i]), name


def test_conv2d_wider_than_the_mfma_kernel_stages_takes_the_scalar_path(dev):
    from neuralmonkey_amd import ops
    g = torch.Generator().manual_seed(19)
    x = torch.randn(1, 10, 11, 3, generator=g).to(dev)
    wd = (torch.randn(9, 9, 3, 4, generator=g) / 15.0).to(dev)
    bd = torch.zeros(4, device=dev)
    y = torch.full((1, 10, 11, 4), NAN, device=dev)
    ops.conv2d_fwd(x, wd, bd, y, "same")
    torch.cuda.synchronize()
    xa, wa = x.double().cpu(), wd.double().cpu()
    _within(y, _conv64(xa, wa, bd.double().cpu(), "same"), _conv64(xa.abs(), wa.abs(), None, "same"), "k = 9")


# ---- batch norm ------------------------------------------------------------------------------------------------------------
BN_SHAPES = [(30, 7), (4290, 12), (4290, 70)]


def _bn_operands(rows, c, dev):
    """Channels 0, 3, 6, ... have mean 10 and deviation 0.1: E[x^2] - E[x]^2 in float32 loses their variance."""
    g = torch.Generator().manual_seed(23)
    x = torch.randn(rows, c, generator=g)
    x[:, ::3] = 10.0 + 0.1 * x[:, ::3]
    gamma = 1.0 + 0.2 * torch.randn(c, generator=g)
    beta = 0.3 * torch.randn(c, generator=g)
    x_full, xd = _padded((rows, c), 3, dev)
    xd.copy_(x)
    return x_full, xd, gamma.to(dev), beta.to(dev)


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "{}x{}".format(*s))
def test_batch_norm_training_forward_and_moving_update(dev, shape, relu):
    """Bounds.  mean: the recipe on |x|.  Variance (two passes): the deviations d = x - mean carry the rounding of x
    (1e-6 |x| is generous), so d^2 is off by 2 |d| 1e-6 |x| -- scale var + 2 sqrt(var) mean|x|; a one-pass variance is
    off by 1e-6 E[x^2], fifty times that for the channels around 10.  y: the recipe on absolute operands."""
    from neuralmonkey_amd import ops
    rows, c = shape
    x_full, xd, gamma, beta = _bn_operands(rows, c, dev)
    x, g64, b64 = xd.double().cpu(), gamma.double().cpu(), beta.double().cpu()
    mm0 = torch.linspace(-1, 1, c)
    mv0 = torch.linspace(0.5, 2, c)
    mm, mv = mm0.to(dev), mv0.to(dev)
    mean, var = torch.full((c,), NAN, device=dev), torch.full((c,), NAN, device=dev)
    y_full, y = _padded((rows, c), 2, dev)
    ops.bn2d_fwd(xd, gamma, beta, y, True, relu, moving_mean=mm, moving_var=mv, batch_mean=mean, batch_var=var)
    torch.cuda.synchronize()
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
    # moving = 0.99 moving + 0.01 batch, the variance that goes in being the UNBIASED one
    unbiased = ref_var * rows / (rows - 1)
    _within(mm, 0.99 * mm0.double() + 0.01 * ref_mean, 0.99 * mm0.double().abs() + 0.01 * ref_mean.abs(), "moving mean")
    _within(mv, 0.99 * mv0.double() + 0.01 * unbiased, 0.99 * mv0.double() + 0.01 * unbiased, "moving variance")
    if rows == 30:                                # 30 / 29: 3.4 % more than the biased variance would have fed in
        assert float(((mv.double().cpu() - 0.99 * mv0.double()) / 0.01 / ref_var).mean()) == pytest.approx(
            rows / (rows - 1), rel=1e-2)
    # without the pointers nothing moves; a second run is bit-equal
    y3 = torch.full((rows, c), NAN, device=dev)
    mean3, var3 = torch.empty_like(mean), torch.empty_like(var)
    ops.bn2d_fwd(xd, gamma, beta, y3, True, relu, batch_mean=mean3, batch_var=var3)
    torch.cuda.synchronize()
    assert torch.equal(y3, y) and torch.equal(mean3, mean) and torch.equal(var3, var)


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "{}x{}".format(*s))
def test_batch_norm_inference_uses_the_moving_statistics(dev, shape, relu):
    from neuralmonkey_amd import ops
    rows, c = shape
    _, xd, gamma, beta = _bn_operands(rows, c, dev)
    mm = torch.linspace(-1, 10, c).to(dev)
    mv = torch.linspace(0.01, 2, c).to(dev)
    keep = (mm.clone(), mv.clone())
    y = torch.full((rows, c), NAN, device=dev)
    ops.bn2d_fwd(xd, gamma, beta, y, False, relu, moving_mean=mm, moving_var=mv)
    torch.cuda.synchronize()
    x, g64, b64, m64, v64 = (t.double().cpu() for t in (xd, gamma, beta, mm, mv))
    ref = TF.batch_norm(x, m64, v64, g64, b64, training=False, eps=M.EPSILON)
    ref = torch.relu(ref) if relu else ref
    _within(y, ref, g64.abs() * (x.abs() + m64.abs()) / torch.sqrt(v64 + M.EPSILON) + b64.abs(), "y")
    assert np.abs(M.np_batch_norm(x.numpy(), g64.numpy(), b64.numpy(), m64.numpy(), v64.numpy())
                  - TF.batch_norm(x, m64, v64, g64, b64, training=False, eps=M.EPSILON).numpy()).max() < 1e-10
    assert torch.equal(mm, keep[0]) and torch.equal(mv, keep[1])                 # read, never written


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "{}x{}".format(*s))
def test_batch_norm_backward_within_four_times_float32_torch(dev, shape, relu):
    """dx = gamma rstd (g - mean(g) - xhat mean(g xhat)) cancels, so the absolute-operand bound says nothing.  The bound
    is instead 4 x the largest error of a float32 torch evaluation on the CPU against float64 on the same inputs, per
    output (dx, dgamma, dbeta), plus the 1e-7 floor.  The float32 CPU evaluation's largest errors on this file's operands
    (plain / with ReLU; the gradients themselves reach 24 .. 51, 6 .. 160 and 8 .. 210):
      30 x 7:     dx 2.7e-5 / 2.1e-5, dgamma 3.1e-5 / 2.7e-5, dbeta 7.8e-7 / 2.8e-7
      4290 x 12:  dx 8.7e-6 / 7.8e-6, dgamma 3.5e-4 / 4.9e-4, dbeta 3.9e-5 / 2.4e-5
      4290 x 70:  dx 1.8e-5 / 1.4e-5, dgamma 2.1e-3 / 1.3e-3, dbeta 7.5e-5 / 4.4e-5
    so the bounds are four times these.  (torch's CPU kernels sum in double, which is why the kernels here do too.)"""
    from neuralmonkey_amd import ops
    rows, c = shape
    _, xd, gamma, beta = _bn_operands(rows, c, dev)
    g = torch.Generator().manual_seed(29)
    dy_full, dyd = _padded((rows, c), 1, dev)
    dyd.copy_(torch.randn(rows, c, generator=g))
    mean, var = torch.empty(c, device=dev), torch.empty(c, device=dev)
    y = torch.empty(rows, c, device=dev)
    ops.bn2d_fwd(xd, gamma, beta, y, True, relu, batch_mean=mean, batch_var=var)

    def torch_grads(dtype):
        p = [t.detach().cpu().to(dtype).requires_grad_(True) for t in (xd, gamma, beta)]
        out = TF.batch_norm(p[0], None, None, p[1], p[2], training=True, eps=M.EPSILON)
        out = torch.relu(out) if relu else out
        out.backward(dyd.cpu().to(dtype))
        return [t.grad.double() for t in p], out.detach()
    want, out64 = torch_grads(torch.float64)
    single, _ = torch_grads(torch.float32)
    bounds = [4 * float((s - w).abs().max()) + 1e-7 for s, w in zip(single, want)]
    print("bn bwd {}x{} relu={}: float32 torch errors {}".format(rows, c, relu, ["{:.2e}".format(b / 4) for b in bounds]))
    # a ReLU input within rounding of zero may be gated differently: such elements are left out of dx, and the test's
    # operands put none of them where it would move the sums beyond their bounds
    safe = torch.ones(rows, c, dtype=torch.bool) if not relu else (out64.abs() > 1e-5) | (out64 == 0) & (
        TF.batch_norm(xd.double().cpu(), None, None, gamma.double().cpu(), beta.double().cpu(), training=True,
                      eps=M.EPSILON) < -1e-5)

    def run(accumulate):
        start = (0.5, 0.125, 0.25) if accumulate else (NAN,) * 3
        dx_full, dx = _padded((rows, c), 2, dev)
        dx.fill_(start[0])
        dg, db = torch.full((c,), start[1], device=dev), torch.full((c,), start[2], device=dev)
        sums = torch.full((2 * c,), NAN, device=dev)
        ops.bn2d_bwd(xd, y if relu else None, dyd, gamma, mean, var, relu, sums, dx=dx, accumulate_dx=accumulate,
                     dgamma=dg, dbeta=db, accumulate_params=accumulate)
        torch.cuda.synchronize()
        return dx_full, dx, dg, db, sums
    dx_full, dx, dg, db, sums = run(False)
    for got, ref, bound, name in ((dx, want[0], bounds[0], "dx"), (dg, want[1], bounds[1], "dgamma"),
                                  (db, want[2], bounds[2], "dbeta")):
        err = (got.double().cpu() - ref).abs()
        if name == "dx":
            err = err[safe]
        print("bn bwd {}: error {:.3e}, bound {:.3e}".format(name, float(err.max()), bound))
        assert float(err.max()) <= bound, "{}: {:.3e} over {:.3e}".format(name, float(err.max()), bound)
    assert _untouched(dx_full, c) and torch.equal(sums[:c], db) and torch.equal(sums[c:], dg)
    _, dx2, dg2, db2, _ = run(False)
    assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2)           # bit-equal
    _, dx3, dg3, db3, _ = run(True)
    assert float((dx3 - 0.5 - dx).abs().max()) <= 1e-6 * (0.5 + float(dx.abs().max()))
    assert float((dg3 - 0.125 - dg).abs().max()) <= 1e-6 * (0.125 + float(dg.abs().max()))
    assert float((db3 - 0.25 - db).abs().max()) <= 1e-6 * (0.25 + float(db.abs().max()))


# ---- windows ---------------------------------------------------------------------------------------------------------------
WINDOW_CASES = [(15, 127, (2, 2), (2, 2)), (15, 127, (2, 2), (1, 1)), (7, 9, (3, 3), (2, 2)), (6, 5, (6, 5), (1, 1))]


def _pool64(x, window, stride, mode):
    xc = x.permute(0, 3, 1, 2)
    out = TF.max_pool2d(xc, window, stride) if mode == "max" else TF.avg_pool2d(xc, window, stride)
    return out.permute(0, 2, 3, 1)


@pytest.mark.parametrize("mode", ["max", "avg"])
@pytest.mark.parametrize("c", [1, 12])
@pytest.mark.parametrize("case", WINDOW_CASES, ids=lambda s: "{}x{}-w{}-s{}".format(s[0], s[1], s[2], s[3]).replace(" ", ""))
def test_window2d_forward_and_gradient_match_float64(dev, case, c, mode):
    from neuralmonkey_amd import ops
    h, w, window, stride = case
    bsz = 2
    g = torch.Generator().manual_seed(31)
    x_full, xd = _padded((bsz, h, w, c), 3, dev)
    xd.copy_(torch.randn(bsz, h, w, c, generator=g))
    oh, ow = ops.window2d_out_hw(h, w, window, stride, "valid")
    y_full, y = _padded((bsz, oh, ow, c), 2, dev)
    argmax = torch.full((bsz, oh, ow, c), -7, dtype=torch.int32, device=dev) if mode == "max" else None
    ops.window2d_fwd(mode, xd, y, window, stride, "valid", argmax=argmax)
    x64 = xd.double().cpu().requires_grad_(True)
    ref = _pool64(x64, window, stride, mode)
    torch.cuda.synchronize()
    assert tuple(ref.shape) == (bsz, oh, ow, c) and _untouched(y_full, c)
    ref_np, where = M.np_window2d(x64.detach().numpy(), window, stride, "valid", mode)
    assert np.abs(ref_np - ref.detach().numpy()).max() < 1e-12
    if mode == "max":
        assert torch.equal(y.cpu().double(), ref.detach())                     # a maximum is exact
        assert np.array_equal(argmax.cpu().numpy(), where)
    else:
        _within(y, ref.detach(), _pool64(x64.detach().abs(), window, stride, "avg"), "y")
    dy_full, dyd = _padded((bsz, oh, ow, c), 1, dev)
    dyd.copy_(torch.randn(bsz, oh, ow, c, generator=g))
    ref.backward(dyd.double().cpu())
    a = x64.detach().abs().requires_grad_(True)
    _pool64(a, window, stride, "avg").backward(dyd.double().cpu().abs())
    scale = a.grad * (window[0] * window[1] if mode == "max" else 1.0)          # every window that reads the position
    for accumulate in (False, True):
        dx_full, dx = _padded((bsz, h, w, c), 4, dev)
        dx.fill_(0.5 if accumulate else NAN)
        ops.window2d_bwd(mode, dyd, dx, window, stride, "valid", argmax=argmax, accumulate=accumulate)
        torch.cuda.synchronize()
        _within(dx - (0.5 if accumulate else 0.0), x64.grad, scale + (0.5 if accumulate else 0.0), "dx")
        assert _untouched(dx_full, c)


def test_window2d_ties_go_to_the_first_maximum_in_row_major_order(dev):
    from neuralmonkey_amd import ops
    x = torch.zeros(1, 4, 4, 2)
    x[0, :, :, 0] = torch.tensor([[3., 3., 1., 5.], [3., 3., 5., 1.], [0., 7., 7., 7.], [7., 0., 7., 7.]])
    x[0, :, :, 1] = -2.0                                                   # all equal, and negative
    xd = x.to(dev)
    y = torch.full((1, 2, 2, 2), NAN, device=dev)
    argmax = torch.zeros((1, 2, 2, 2), dtype=torch.int32, device=dev)
    ops.window2d_fwd("max", xd, y, (2, 2), (2, 2), "valid", argmax=argmax)
    dy = torch.tensor([[[[1., 10.], [2., 20.]], [[3., 30.], [4., 40.]]]]).to(dev)
    dx = torch.full((1, 4, 4, 2), NAN, device=dev)
    ops.window2d_bwd("max", dy, dx, (2, 2), (2, 2), "valid", argmax=argmax)
    torch.cuda.synchronize()
    assert y[0, :, :, 0].cpu().tolist() == [[3., 5.], [7., 7.]] and bool((y[..., 1] == -2.0).all())
    assert argmax[0, :, :, 0].cpu().tolist() == [[0, 3], [9, 10]] and argmax[0, :, :, 1].cpu().tolist() == [[0, 2], [8, 10]]
    want = torch.zeros(4, 4)
    want[0, 0], want[0, 3], want[2, 1], want[2, 2] = 1., 2., 3., 4.
    assert torch.equal(dx[0, :, :, 0].cpu(), want)
    want1 = torch.zeros(4, 4)
    want1[0, 0], want1[0, 2], want1[2, 0], want1[2, 2] = 10., 20., 30., 40.
    assert torch.equal(dx[0, :, :, 1].cpu(), want1)
    # overlapping windows (stride 1): a position that is the first maximum of several windows collects them all
    y2 = torch.empty(1, 3, 3, 2, device=dev)
    arg2 = torch.zeros((1, 3, 3, 2), dtype=torch.int32, device=dev)
    ops.window2d_fwd("max", xd, y2, (2, 2), (1, 1), "valid", argmax=arg2)
    dx2 = torch.full((1, 4, 4, 2), NAN, device=dev)
    ops.window2d_bwd("max", torch.ones(1, 3, 3, 2, device=dev), dx2, (2, 2), (1, 1), "valid", argmax=arg2)
    torch.cuda.synchronize()
    _, where = M.np_window2d(x.double().numpy(), (2, 2), (1, 1), "valid", "max")
    assert np.array_equal(arg2.cpu().numpy(), where)
    counts = np.zeros((16, 2))
    for ch in range(2):
        np.add.at(counts[:, ch], where[0, :, :, ch].reshape(-1), 1.0)
    assert np.array_equal(dx2[0].cpu().numpy().reshape(16, 2), counts)


@pytest.mark.parametrize("case", [(7, 9, (3, 3), (2, 2)), (5, 8, (2, 2), (1, 1)), (6, 6, (3, 3), (1, 1)),
                                  (15, 127, (2, 2), (2, 2))],
                         ids=lambda s: "{}x{}-w{}-s{}".format(s[0], s[1], s[2], s[3]).replace(" ", ""))
def test_window2d_same_padding_pools_a_mask_as_tensorflow_does(dev, case):
    """C = 1, no gradient: the mask of a "same" convolution (cnn_encoder.py:238) against the NumPy restatement, whose
    SAME arithmetic test_cnn2d_host.py pins; padded positions take no part, in the average either."""
    from neuralmonkey_amd import ops
    h, w, window, stride = case
    g = torch.Generator().manual_seed(37)
    mask = (torch.rand(3, h, w, 1, generator=g) > 0.6).float()
    mask[1, :, w // 2:] = 0.0
    oh, ow = ops.window2d_out_hw(h, w, window, stride, "same")
    assert (oh, ow) == (M.np_pad(h, window[0], stride[0], "same")[0], M.np_pad(w, window[1], stride[1], "same")[0])
    md = mask.to(dev)
    for mode in ("max", "avg"):
        out = torch.full((3, oh, ow, 1), NAN, device=dev)
        ops.window2d_fwd(mode, md, out, window, stride, "same")
        torch.cuda.synchronize()
        want, _ = M.np_window2d(mask.double().numpy(), window, stride, "same", mode)
        if mode == "max":
            assert np.array_equal(out.cpu().numpy(), want)
        else:
            assert np.abs(out.cpu().numpy() - want).max() <= 2e-7
            dx = torch.full((3, h, w, 1), NAN, device=dev)
            ops.window2d_bwd("avg", torch.ones_like(out), dx, window, stride, "same")
            torch.cuda.synchronize()
            assert abs(float(dx.sum()) - out.numel()) < 1e-3 * out.numel()          # every window hands out exactly 1


def test_map_columns_and_back(dev):
    from neuralmonkey_amd import ops
    g = torch.Generator().manual_seed(41)
    x = torch.randn(3, 4, 7, 5, generator=g).to(dev)
    cols = torch.full((3, 7, 20), NAN, device=dev)
    ops.map_columns(x, cols)
    back = torch.full((3, 4, 7, 5), NAN, device=dev)
    ops.map_columns(cols, back, inverse=True)
    torch.cuda.synchronize()
    assert torch.equal(cols.cpu(), x.cpu().permute(0, 2, 1, 3).reshape(3, 7, 20)) and torch.equal(back, x)


# ---- taped functions -------------------------------------------------------------------------------------------------------
class _Ctx:                       # the tape needs buffers only
    def __init__(self, dev):
        self.device = dev
        self.session = type("Session", (), {})()

    def buffer(self, key, shape, dtype=torch.float32, zero=False):
        return torch.zeros(shape, dtype=dtype, device=self.device)


def test_taped_image_functions_match_float64_autograd(dev):
    """conv2d (valid) -> batch_norm2d + ReLU = a; conv2d (same, k 2) of a PLUS a (a Var with two readers) -> max window
    -> global average, on a tape: values and every gradient."""
    from neuralmonkey_amd import autodiff as F
    from neuralmonkey_amd import image_ops as I
    g = torch.Generator().manual_seed(43)
    bsz, h, w, cin, c = 3, 7, 9, 2, 5
    x = torch.randn(bsz, h, w, cin, generator=g, dtype=torch.float64)
    w1 = torch.randn(3, 3, cin, c, generator=g, dtype=torch.float64) / 4
    b1 = torch.randn(c, generator=g, dtype=torch.float64) * 0.3
    gamma = 1 + 0.2 * torch.randn(c, generator=g, dtype=torch.float64)
    beta = 0.3 * torch.randn(c, generator=g, dtype=torch.float64)
    w2 = torch.randn(2, 2, c, c, generator=g, dtype=torch.float64) / 4
    b2 = torch.randn(c, generator=g, dtype=torch.float64) * 0.3
    d_out = torch.randn(bsz, c, generator=g, dtype=torch.float64)
    f32 = lambda t: t.float().contiguous().to(dev)
    tape = F.Tape(_Ctx(dev), "image", recording=True)
    v = lambda t: F.Var(f32(t), torch.zeros_like(f32(t)), True)
    xv = F.Var(f32(x).view(bsz * h * w, cin), None, True)
    xv.is_leaf = True
    params = [v(t) for t in (w1, b1, gamma, beta, w2, b2)]
    mm, mv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
    t1, shape = I.conv2d(tape, xv, params[0], params[1], (bsz, h, w), "valid")
    a, (mean, var) = I.batch_norm2d(tape, t1, params[2], params[3], mm, mv, True, True, update_moving=True)
    t2, _ = I.conv2d(tape, a, params[4], params[5], shape, "same")
    s = F.add(tape, t2, a)
    pooled, pshape = I.window2d(tape, "max", s, shape, (2, 2), (2, 2))
    out, oshape = I.window2d(tape, "avg", pooled, pshape, pshape[1:], (1, 1))
    assert shape == (bsz, 5, 7) and pshape == (bsz, 2, 3) and oshape == (bsz, 1, 1)
    F.ops.ew("copy", f32(d_out), None, tape.grad(out), accumulate=True)
    tape.backward()
    torch.cuda.synchronize()

    p = [t.clone().requires_grad_(True) for t in (x, w1, b1, gamma, beta, w2, b2)]
    r1 = _conv64(p[0], p[1], p[2], "valid")
    ra = torch.relu(TF.batch_norm(r1.reshape(-1, c), None, None, p[3], p[4], training=True, eps=M.EPSILON)).view(r1.shape)
    rs = _conv64(ra, p[5], p[6], "same") + ra
    rp = _pool64(rs, (2, 2), (2, 2), "max")
    ref = rp.mean(dim=(1, 2))
    (ref * d_out).sum().backward()
    assert float((out.data.double().cpu() - ref.detach()).abs().max()) < 1e-5 * float(ref.detach().abs().max())
    assert float((mean.double().cpu() - r1.detach().mean(dim=(0, 1, 2))).abs().max()) < 1e-5
    n = bsz * 5 * 7
    assert float((mv.double().cpu() - (0.99 + 0.01 * r1.detach().reshape(-1, c).var(0, unbiased=True))).abs().max()) < 1e-5
    assert float((mm.double().cpu() - 0.01 * r1.detach().mean(dim=(0, 1, 2))).abs().max()) < 1e-6 and n > 1
    got = [xv.grad.view(bsz, h, w, cin)] + [q.grad for q in params]
    for mine, want, name in zip(got, p, ("x", "w1", "b1", "gamma", "beta", "w2", "b2")):
        err = (mine.double().cpu() - want.grad).abs().max() / (want.grad.abs().max() + 1e-12)
        # (b1 shifts every pre-activation of a channel alike and batch norm removes the shift: its gradient is zero
        # up to rounding, so it is measured against the other gradients' magnitude)
        if name == "b1":
            err = (mine.double().cpu() - want.grad).abs().max() / p[4].grad.abs().max()
        assert float(err) < 2e-5, (name, float(err))


# entry point of include/nmhip_image.h -> the tests of this file that call it
ENTRY_POINTS = {
    "nm_conv2d_fwd": ["test_conv2d_forward_and_gradients_match_float64", "test_conv2d_algos_agree_and_auto_is_one_of_them",
                      "test_conv2d_wider_than_the_mfma_kernel_stages_takes_the_scalar_path",
                      "test_taped_image_functions_match_float64_autograd"],
    "nm_conv2d_workspace_bytes": ["test_conv2d_forward_and_gradients_match_float64",
                                  "test_taped_image_functions_match_float64_autograd"],
    "nm_conv2d_bwd": ["test_conv2d_forward_and_gradients_match_float64", "test_conv2d_algos_agree_and_auto_is_one_of_them",
                      "test_taped_image_functions_match_float64_autograd"],
    "nm_bn2d_fwd": ["test_batch_norm_training_forward_and_moving_update",
                    "test_batch_norm_inference_uses_the_moving_statistics",
                    "test_taped_image_functions_match_float64_autograd"],
    "nm_bn2d_bwd": ["test_batch_norm_backward_within_four_times_float32_torch",
                    "test_taped_image_functions_match_float64_autograd"],
    "nm_window2d_fwd": ["test_window2d_forward_and_gradient_match_float64",
                        "test_window2d_ties_go_to_the_first_maximum_in_row_major_order",
                        "test_window2d_same_padding_pools_a_mask_as_tensorflow_does",
                        "test_taped_image_functions_match_float64_autograd"],
    "nm_window2d_bwd": ["test_window2d_forward_and_gradient_match_float64",
                        "test_window2d_ties_go_to_the_first_maximum_in_row_major_order",
                        "test_taped_image_functions_match_float64_autograd"],
    "nm_map_columns": ["test_map_columns_and_back"],
}


def test_every_entry_point_has_a_test(dev):
    from neuralmonkey_amd import _lib
    assert set(ENTRY_POINTS) == set(_lib.IMAGE_SIGNATURES)
    assert all(name in globals() for tests in ENTRY_POINTS.values() for name in tests)
