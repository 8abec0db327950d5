"""The point-wise, sequence-utility and backward kernels of the general (taped) path, each called directly and compared
with the float64 evaluation of its plain restatement (oracle/pointwise_ref.py; backward passes: torch.autograd of the
forward restatement) -- at a tiny odd shape, a mid shape with ragged tails and a shape past the first trip of the
kernels' grid-stride loops, contiguous and as column slices of wider buffers (offsets that break 16-byte alignment),
with every optional pointer present and absent and every accumulate flag off (onto NaN, which must be overwritten) and
on (onto a random base).  Buffers carry NaN margins: nothing outside an operand's extent may be written.

Inputs, expected values and bounds come from tests/pointwise_cases.py; tests/test_pointwise_refs.py shows on the CPU that
a float32 evaluation of the same references on the same inputs meets the same bounds.

``LEDGER`` at the end maps every entry point of include/nmhip.h to the test that calls it directly (checked by
tests/test_pointwise_refs.py)."""
import numpy as np
import pytest
import torch

from oracle import pointwise_ref as P
from tests import pointwise_cases as C

pytestmark = pytest.mark.gpu
NAN = float("nan")
LAYOUTS = ("contiguous", "strided")


# ---- buffers with guards -------------------------------------------------------------------------------------------
class Buf:
    """A [rows, cols] float32 device operand inside a NaN-filled buffer.  ``contiguous``: rows back to back, the buffer
    has a margin of 8 floats before and after (the operand stays 16-byte aligned).  ``strided``: a column slice with
    ld = cols + 3 that starts one float into the row: ld > cols and no row is 16-byte aligned."""

    def __init__(self, dev, rows, cols, layout, init=None, dtype=torch.float32):
        self.rows, self.cols = rows, cols
        fill = NAN if dtype == torch.float32 else -77
        if layout == "contiguous":
            self.full = torch.full((rows * cols + 16,), fill, dtype=dtype, device=dev)
            self.view = self.full[8:8 + rows * cols].view(rows, cols)
            self._inside = torch.zeros(rows * cols + 16, dtype=torch.bool)
            self._inside[8:8 + rows * cols] = True
        else:
            self.full = torch.full((rows, cols + 3), fill, dtype=dtype, device=dev)
            self.view = self.full[:, 1:1 + cols]
            self._inside = torch.zeros(rows, cols + 3, dtype=torch.bool)
            self._inside[:, 1:1 + cols] = True
        self.fill = fill
        if init is not None:
            self.view.copy_(torch.as_tensor(np.ascontiguousarray(init)).to(dev))

    def get(self):
        """The operand as a NumPy array, after checking that nothing around it was written."""
        full = self.full.cpu()
        outside = full[~self._inside]
        assert bool(torch.isnan(outside).all() if self.full.dtype == torch.float32 else (outside == self.fill).all()), \
            "written outside the operand"
        return full[self._inside].view(self.rows, self.cols).numpy()


def dev_in(dev, arr, layout):
    """A read-only operand: a Buf holding ``arr`` (reading outside it yields NaN)."""
    arr = np.asarray(arr)
    if arr.ndim == 1:
        arr = arr.reshape(1, -1)
    return Buf(dev, arr.shape[0], arr.shape[1], layout, init=arr).view


def i32(dev, arr):
    return torch.tensor(np.asarray(arr), dtype=torch.int32, device=dev)


def check(got, ref, tol, what):
    """|got - ref| <= tol * max(1, |ref|max); tol 0: bit for bit against the float32 ``ref``."""
    if tol == 0.0:
        assert ref.dtype == np.float32, what
        assert np.array_equal(got, ref, equal_nan=False), "{}: not bit-exact, max diff {}".format(
            what, np.abs(got.astype(np.float64) - ref).max())
        return
    err, bnd = C.max_err(got, C.np64(ref)), C.bound(tol, C.np64(ref))
    print("{}: err {:.3g} bound {:.3g}".format(what, err, bnd))
    assert err <= bnd, "{}: err {:.3g} > bound {:.3g}".format(what, err, bnd)


# ---- nm_ew ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", P.EW_OPS)
def test_ew_every_op_code(dev, op):
    """All 15 op codes at the four shapes (the float4 kernel and the scalar kernel both past their first trip),
    contiguous / unaligned-contiguous / strided, written onto NaN and accumulated onto a base.  Single correctly-rounded
    operations are compared bit for bit with float32 NumPy; the rest with float64 (1e-6).  An accumulating call adds the
    result to the base: the add may be contracted into an fma, so it is compared with float64."""
    from neuralmonkey_amd import ops
    alpha = C.EW_ALPHA.get(op, 0.0)
    for shape in C.EW_SHAPES:
        rows, cols = shape
        a, b, base = C.ew_inputs(op, shape)
        ref64 = C.ew_expect(op, a, b, np.float64)
        ref = P.ew(op, a, b, alpha) if C.ew_tol(op) == 0.0 else ref64
        big = rows * cols > (1 << 20)
        # [6400, 1536]: contiguous (float4 kernel); [6400, 1535]: strided (scalar kernel at the same size)
        layouts = (("contiguous",) if cols == 1536 else ("strided",)) if big else LAYOUTS
        for layout in layouts:
            ad = dev_in(dev, a, layout)
            bd = None if b is None else dev_in(dev, b, layout)
            for acc in (False, True):
                out = Buf(dev, rows, cols, layout, init=base if acc else None)
                ops.ew(op, ad, bd, out.view, alpha=alpha, accumulate=acc)
                what = "ew {} {} {} acc={}".format(op, shape, layout, acc)
                if acc:
                    check(out.get(), base.astype(np.float64) + ref64, C.TOL_ACT, what)
                else:
                    check(out.get(), ref, C.ew_tol(op), what)
    # contiguous but NOT 16-byte aligned (one float into an allocation), a multiple of 4 elements: the scalar kernel
    rows, cols = 12, 20
    a, b, _ = C.ew_inputs(op, (rows, cols))
    flat = torch.full((3 * rows * cols + 16,), NAN, device=dev)
    ad = flat[1:1 + rows * cols].view(rows, cols)
    ad.copy_(torch.as_tensor(a))
    bd = None
    if b is not None:
        bd = flat[rows * cols + 2:rows * cols + 2 + b.size].view(b.shape)
        bd.copy_(torch.as_tensor(b))
    od = flat[2 * rows * cols + 5:3 * rows * cols + 5].view(rows, cols)
    ops.ew(op, ad, bd, od, alpha=alpha)
    ref = P.ew(op, a, b, alpha) if C.ew_tol(op) == 0.0 else C.ew_expect(op, a, b, np.float64)
    check(od.cpu().numpy(), ref, C.ew_tol(op), "ew {} unaligned".format(op))
    assert bool(torch.isnan(flat[3 * rows * cols + 5:]).all()) and bool(torch.isnan(flat[0]))


def test_ew_saturates_and_handles_infinities(dev):
    """tanh / sigmoid at |x| of 30 .. 100 (exp overflows) give exactly +-1 / 0 / 1, never NaN; logaddexp with -inf on
    both sides gives -inf."""
    from neuralmonkey_amd import ops
    x = np.array([[30.0, -30.0, 88.0, -88.0, 89.0, -89.0, 100.0, -100.0, 1e4, -1e4]], dtype=np.float32)
    xd = torch.tensor(x, device=dev)
    t = ops.ew("tanh", xd, None, torch.empty_like(xd)).cpu().numpy()
    assert np.array_equal(t, np.sign(x))
    s = ops.ew("sigmoid", xd, None, torch.empty_like(xd), alpha=0.0).cpu().numpy()
    assert np.isfinite(s).all() and np.array_equal(s[x > 0], np.ones(5, dtype=np.float32))
    assert np.abs(s[x < 0]).max() <= 1e-12
    ninf = torch.full((1, 7), -np.inf, device=dev)
    assert bool((ops.ew("logaddexp", ninf, ninf, torch.empty_like(ninf)) == -np.inf).all())


# ---- LSTM cell -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,h", C.PW_SHAPES)
def test_lstm_cell_fwd_bwd(dev, rows, h):
    """nm_lstm_cell_fwd / _bwd: forget_bias 0 and 1, gates absent and present, z / dz column blocks of wider buffers,
    saturated gates; backward with dh alone, dc_new alone and both, dc_prev absent / written / accumulated, dz written
    onto NaN / accumulated."""
    from neuralmonkey_amd import ops
    inp = C.lstm_inputs(rows, h)
    combos = [(0.0, "contiguous", True), (1.0, "strided", True), (1.0, "contiguous", False)]
    for fb, layout, with_gates in combos:
        want = C.lstm_expect(inp, fb, np.float64)
        z, c_prev = dev_in(dev, inp["z"], layout), dev_in(dev, inp["c_prev"], layout)
        c_new, h_new = Buf(dev, rows, h, layout), Buf(dev, rows, h, layout)
        gates = Buf(dev, rows, 4 * h, layout) if with_gates else None
        ops.lstm_cell_fwd(z, c_prev, c_new.view, h_new.view, None if gates is None else gates.view, forget_bias=fb)
        what = "lstm {}x{} fb={} {}".format(rows, h, fb, layout)
        check(c_new.get(), want["c_new"], C.TOL_FUSED, what + " c_new")
        check(h_new.get(), want["h_new"], C.TOL_FUSED, what + " h_new")
        if gates is None:
            continue
        check(gates.get(), want["gates"], C.TOL_FUSED, what + " gates")
        # backward from the kernel's own saved gates / cell state (what a model feeds it)
        for use_dh, use_dc in ((True, True), (True, False), (False, True)):
            wb = C.lstm_expect(inp, fb, np.float64, use_dh, use_dc)
            dh = dev_in(dev, inp["dh"], layout) if use_dh else None
            dcn = dev_in(dev, inp["dc_new"], layout) if use_dc else None
            for acc_dz, dcp_mode in ((False, "write"), (True, "acc"), (False, "absent")):
                dz = Buf(dev, rows, 4 * h, layout, init=inp["base_dz"] if acc_dz else None)
                dcp = None if dcp_mode == "absent" else Buf(dev, rows, h, layout,
                                                            init=inp["base_dc"] if dcp_mode == "acc" else None)
                ops.lstm_cell_bwd(dh, dcn, gates.view, c_prev, c_new.view, dz.view, None if dcp is None else dcp.view,
                                  accumulate_dz=acc_dz, accumulate_dc_prev=dcp_mode == "acc")
                w2 = "{} bwd dh={} dc={} acc_dz={} dc_prev={}".format(what, use_dh, use_dc, acc_dz, dcp_mode)
                check(dz.get(), C.np64(wb["dz"]) + (inp["base_dz"] if acc_dz else 0.0), C.TOL_FUSED, w2 + " dz")
                if dcp is not None:
                    check(dcp.get(), C.np64(wb["dc_prev"]) + (inp["base_dc"] if dcp_mode == "acc" else 0.0),
                          C.TOL_FUSED, w2 + " dc_prev")


# ---- NematusGRU cell -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,h", C.PW_SHAPES)
def test_nematus_cell_fwd_bwd(dev, rows, h):
    """nm_nematus_cell_fwd / _bwd with and without g2 / dg2 (dg2 must equal what dg received, bit for bit); dci, dsc,
    dh_prev each absent / written / accumulated; the ru and c_out the forward saved feed the backward."""
    from neuralmonkey_amd import ops
    inp = C.nematus_inputs(rows, h)
    for with_g2, layout in ((False, "contiguous"), (True, "strided"), (True, "contiguous")):
        want = C.nematus_expect(inp, with_g2, np.float64)
        g_pre, sc, ci = (dev_in(dev, inp[k], layout) for k in ("g_pre", "sc", "ci"))
        h_prev, dh = dev_in(dev, inp["h_prev"], layout), dev_in(dev, inp["dh"], layout)
        g2 = dev_in(dev, inp["g2"], layout) if with_g2 else None
        h_new = Buf(dev, rows, h, layout)
        ru, c_out = Buf(dev, rows, 2 * h, "contiguous"), Buf(dev, rows, h, "contiguous")
        ops.nematus_cell_fwd(g_pre, sc, ci, h_prev, h_new.view, ru=ru.view, c_out=c_out.view, g2=g2)
        what = "nematus {}x{} g2={} {}".format(rows, h, with_g2, layout)
        check(h_new.get(), want["h_new"], C.TOL_FUSED, what + " h_new")
        check(ru.get(), want["ru"], C.TOL_FUSED, what + " ru")
        check(c_out.get(), want["c"], C.TOL_FUSED, what + " c")
        h_only = Buf(dev, rows, h, layout)                       # without the saved activations: the same h'
        ops.nematus_cell_fwd(g_pre, sc, ci, h_prev, h_only.view, g2=g2)
        assert np.array_equal(h_only.get(), h_new.get()), what
        # modes of (dci, dsc, dh_prev): every one of them absent / written / accumulated at least once
        for modes in (("write", "write", "write"), ("acc", "acc", "acc"), ("absent", "write", "acc"),
                      ("write", "absent", "absent"), ("acc", "write", "absent")):
            for acc_dg in (False, True):
                if acc_dg and modes[0] != "acc":
                    continue
                dg = Buf(dev, rows, 2 * h, layout, init=inp["base_dg"] if acc_dg else None)
                dg2 = Buf(dev, rows, 2 * h, layout) if with_g2 else None
                outs = {}
                for name, base, mode in zip(("dci", "dsc", "dh_prev"), ("base_dci", "base_dsc", "base_dhp"), modes):
                    outs[name] = None if mode == "absent" else Buf(dev, rows, h, layout,
                                                                   init=inp[base] if mode == "acc" else None)
                v = lambda b_: None if b_ is None else b_.view
                ops.nematus_cell_bwd(dh, ru.view, c_out.view, sc, h_prev, dg.view, v(outs["dci"]), v(outs["dsc"]),
                                     v(outs["dh_prev"]), acc_dg=acc_dg, acc_dci=modes[0] == "acc",
                                     acc_dsc=modes[1] == "acc", acc_dh_prev=modes[2] == "acc", dg2=v(dg2))
                w2 = "{} bwd {} acc_dg={}".format(what, modes, acc_dg)
                got_dg = dg.get()
                check(got_dg, C.np64(want["dg"]) + (inp["base_dg"] if acc_dg else 0.0), C.TOL_FUSED, w2 + " dg")
                if dg2 is not None:
                    check(dg2.get(), want["dg"], C.TOL_FUSED, w2 + " dg2")
                    if not acc_dg:
                        assert np.array_equal(dg2.get(), got_dg), w2 + ": dg2 differs from dg"
                for name, base, mode in zip(("dci", "dsc", "dh_prev"), ("base_dci", "base_dsc", "base_dhp"), modes):
                    if outs[name] is not None:
                        check(outs[name].get(), C.np64(want[name]) + (inp[base] if mode == "acc" else 0.0), C.TOL_FUSED,
                              "{} {}".format(w2, name))


def test_nematus_cell_dg2_equals_the_increment_of_dg(dev):
    """With accumulate_dg the second destination receives the step's gradient alone: dg - base == dg2 up to the
    rounding of the one add."""
    from neuralmonkey_amd import ops
    rows, h = C.MID
    inp = C.nematus_inputs(rows, h)
    t = lambda k: torch.tensor(inp[k], device=dev)
    ru, c = torch.empty(rows, 2 * h, device=dev), torch.empty(rows, h, device=dev)
    ops.nematus_cell_fwd(t("g_pre"), t("sc"), t("ci"), t("h_prev"), torch.empty(rows, h, device=dev), ru=ru, c_out=c,
                         g2=t("g2"))
    dg, dg2, plain = t("base_dg"), torch.full((rows, 2 * h), NAN, device=dev), torch.full((rows, 2 * h), NAN, device=dev)
    ops.nematus_cell_bwd(t("dh"), ru, c, t("sc"), t("h_prev"), dg, None, None, None, acc_dg=True, dg2=dg2)
    ops.nematus_cell_bwd(t("dh"), ru, c, t("sc"), t("h_prev"), plain, None, None, None)
    assert torch.equal(dg2, plain)
    assert torch.equal(dg, t("base_dg") + plain)


# ---- blend ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", C.PW_SHAPES)
def test_blend_fwd_bwd(dev, rows, cols):
    """nm_blend_fwd / _bwd: each of du, dh, dc absent in turn; the present ones accumulate onto a non-zero base."""
    from neuralmonkey_amd import ops
    inp = C.blend_inputs(rows, cols)
    want = C.blend_expect(inp, np.float64)
    for layout in LAYOUTS:
        u, h, c, dy = (dev_in(dev, inp[k], layout) for k in ("u", "h", "c", "dy"))
        out = Buf(dev, rows, cols, layout)
        ops.blend_fwd(u, h, c, out.view)
        check(out.get(), want["out"], C.TOL_ACT, "blend {}x{} {}".format(rows, cols, layout))
        for absent in (None, "du", "dh", "dc"):
            bufs = {k: (None if k == absent else Buf(dev, rows, cols, layout, init=inp["base_" + k]))
                    for k in ("du", "dh", "dc")}
            v = lambda b_: None if b_ is None else b_.view
            ops.blend_bwd(dy, u, h, c, v(bufs["du"]), v(bufs["dh"]), v(bufs["dc"]))
            for k, b_ in bufs.items():
                if b_ is not None:
                    check(b_.get(), C.np64(want[k]) + inp["base_" + k], C.TOL_ACT,
                          "blend_bwd {}x{} {} without {}: {}".format(rows, cols, layout, absent, k))


# ---- rnn_select ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", C.PW_SHAPES)
def test_rnn_select_fwd_bwd(dev, rows, cols):
    """nm_rnn_select_*: lengths 0, t, t + 1 and far past the last step, and lengths=None; y_out / dy / dh / d_prev absent.
    The forward is a select: bit for bit (dead rows pass h_prev through).  The backward adds onto a base."""
    from neuralmonkey_amd import ops
    inp = C.select_inputs(rows, cols)
    for layout in LAYOUTS:
        h_new, h_prev, dh, dy = (dev_in(dev, inp[k], layout) for k in ("h_new", "h_prev", "dh", "dy"))
        for lengths in (True, False):
            ln = i32(dev, inp["lengths"]) if lengths else None
            want = C.select_expect(inp, np.float32, lengths)
            for with_y in (True, False):
                h_out = Buf(dev, rows, cols, layout)
                y_out = Buf(dev, rows, cols, layout) if with_y else None
                ops.rnn_select_fwd(h_new, h_prev, ln, C.SELECT_T, h_out.view, None if y_out is None else y_out.view)
                what = "select {}x{} {} lengths={}".format(rows, cols, layout, lengths)
                check(h_out.get(), want["h_out"].numpy(), 0.0, what + " h_out")
                if with_y:
                    check(y_out.get(), want["y_out"].numpy(), 0.0, what + " y_out")
            if lengths:
                dead = inp["lengths"] <= C.SELECT_T
                assert dead.any() and np.array_equal(h_out.get()[dead], inp["h_prev"][dead])
            for use_dh, use_dy, with_prev in ((True, True, True), (False, True, True), (True, False, True),
                                              (True, True, False)):
                wb = C.select_expect(inp, np.float64, lengths, use_dh, use_dy)
                d_new = Buf(dev, rows, cols, layout, init=inp["base_new"])
                d_prev = Buf(dev, rows, cols, layout, init=inp["base_prev"]) if with_prev else None
                ops.rnn_select_bwd(dh if use_dh else None, dy if use_dy else None, ln, C.SELECT_T, d_new.view,
                                   None if d_prev is None else d_prev.view)
                w2 = "{} bwd dh={} dy={} d_prev={}".format(what, use_dh, use_dy, with_prev)
                check(d_new.get(), C.np64(wb["d_new"]) + inp["base_new"], C.TOL_ACT, w2 + " d_new")
                if with_prev:
                    check(d_prev.get(), C.np64(wb["d_prev"]) + inp["base_prev"], C.TOL_ACT, w2 + " d_prev")


# ---- reverse_sequence ----------------------------------------------------------------------------------------------
def _flat_guard(dev, n, init=None, dtype=torch.float32):
    """n contiguous elements with 8 guard elements on either side."""
    fill = NAN if dtype == torch.float32 else -77
    full = torch.full((n + 16,), fill, dtype=dtype, device=dev)
    if init is not None:
        full[8:8 + n].copy_(torch.as_tensor(np.ascontiguousarray(init).reshape(-1)))
    return full, full[8:8 + n]


def _guards_intact(full):
    edge = torch.cat([full[:8], full[-8:]]).cpu()
    return bool(torch.isnan(edge).all()) if full.dtype == torch.float32 else bool((edge == -77).all())


@pytest.mark.parametrize("b,s,d", [(4, 3, 5), (9, 13, 33), (128, 50, 1024)])
def test_reverse_sequence(dev, b, s, d):
    """nm_reverse_sequence: lengths 0, 1, S and beyond S (clamped); a permutation, so bit for bit; applying it twice
    returns the input; accumulate=True (its backward pass) adds onto a base."""
    from neuralmonkey_amd import ops
    rng = np.random.default_rng([b, s, d])
    x = C.normal(rng, (b, s, d))
    lengths = rng.integers(0, s + 4, b).astype(np.int32)
    lengths[:4] = (0, 1, s, s + 5)
    want = P.reverse_sequence(x, lengths)
    for i in range(b):                                    # the restatement against np.flip per sentence
        n = min(int(lengths[i]), s)
        assert np.array_equal(want[i, :n], np.flip(x[i, :n], 0)) and np.array_equal(want[i, n:], x[i, n:])
    xd, ld = torch.tensor(x, device=dev), i32(dev, lengths)
    full, out = _flat_guard(dev, x.size)
    ops.reverse_sequence(xd, out.view(b, s, d), ld)
    assert np.array_equal(out.view(b, s, d).cpu().numpy(), want) and _guards_intact(full)
    full2, back = _flat_guard(dev, x.size)
    ops.reverse_sequence(out.view(b, s, d), back.view(b, s, d), ld)
    assert torch.equal(back.view(b, s, d), xd) and _guards_intact(full2)
    base = C.normal(rng, (b, s, d))
    full3, acc = _flat_guard(dev, x.size, init=base)
    ops.reverse_sequence(xd, acc.view(b, s, d), ld, accumulate=True)
    assert np.array_equal(acc.view(b, s, d).cpu().numpy(), base + want) and _guards_intact(full3)


# ---- maxout --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,groups,pool", [(3, 5, 2), (301, 131, 3), (1031, 1021, 2)])
def test_maxout_fwd_bwd(dev, rows, groups, pool):
    """nm_maxout_fwd / _bwd with pool 2 and 3 on inputs full of ties (the first maximum wins, as MaxPoolGrad), argmax
    absent; the backward adds into a non-zero dx at the argmax positions only."""
    from neuralmonkey_amd import ops
    rng = np.random.default_rng([rows, groups, pool])
    x = (np.round(rng.standard_normal((rows, pool * groups)) * 2.0) / 2.0).astype(np.float32)       # many exact ties
    dy, base = C.normal(rng, (rows, groups)), C.normal(rng, (rows, pool * groups))
    want, arg = P.maxout(torch.tensor(x), pool)
    x3 = x.reshape(rows, pool, groups)
    assert np.array_equal(arg.numpy(), x3.argmax(1)) and (x3 == x3.max(1, keepdims=True)).sum(1).max() > 1
    dx_want = P.maxout_grads(torch.tensor(x, dtype=torch.float64), pool, torch.tensor(dy, dtype=torch.float64)).numpy()
    for layout in LAYOUTS:
        xd, dyd = dev_in(dev, x, layout), dev_in(dev, dy, layout)
        out, out2 = Buf(dev, rows, groups, layout), Buf(dev, rows, groups, layout)
        argd = Buf(dev, rows, groups, "contiguous", dtype=torch.int32)
        ops.maxout_fwd(xd, out.view, argd.view, pool=pool)
        ops.maxout_fwd(xd, out2.view, None, pool=pool)
        what = "maxout {}x{}x{} {}".format(rows, groups, pool, layout)
        check(out.get(), want.numpy(), 0.0, what)
        check(out2.get(), want.numpy(), 0.0, what + " (no argmax)")
        assert np.array_equal(argd.get(), arg.numpy()), what
        dx = Buf(dev, rows, pool * groups, layout, init=base)
        ops.maxout_bwd(dyd, argd.view, dx.view, pool=pool)
        got = dx.get()
        check(got, (base.astype(np.float64) + dx_want).astype(np.float32), 0.0, what + " dx")
        touched = np.zeros((rows, pool, groups), dtype=bool)
        np.put_along_axis(touched, arg.numpy()[:, None, :].astype(np.int64), True, axis=1)
        assert np.array_equal(got.reshape(rows, pool, groups)[~touched], base.reshape(rows, pool, groups)[~touched])


# ---- dropout -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", C.DROPOUT_SHAPES)
def test_dropout_salt_step_accumulate(dev, rows, cols):
    """nm_dropout against the restated mask: written and accumulated, with the step word absent, 0, 1 and large (the
    effective salt is (salt + step * 0x9E3779B9) mod 2^32), keep_prob 1 the identity, masks past 2^20 elements.  The
    kept elements are x * (1 / keep_prob): one multiplication, bit for bit."""
    from neuralmonkey_amd import ops
    x, base = C.dropout_inputs(rows, cols)
    salt, keep = C.DROPOUT_SALT, C.DROPOUT_KEEP
    layouts = ("contiguous",) if cols == 1536 else LAYOUTS
    for layout in layouts:
        xd = dev_in(dev, x, layout)
        for step in (None, 0, 1, 2000000011):
            want = P.dropout(x, keep, salt, step)
            assert 0.6 < float((want != 0).mean()) < 0.8 or rows * cols < 100
            sd = None if step is None else i32(dev, [step])
            out = Buf(dev, rows, cols, layout)
            ops.dropout(xd, out.view, keep, salt, step=sd)
            what = "dropout {}x{} {} step={}".format(rows, cols, layout, step)
            check(out.get(), want, 0.0, what)
            if step in (None, 1):
                acc = Buf(dev, rows, cols, layout, init=base)
                ops.dropout(xd, acc.view, keep, salt, accumulate=True, step=sd)
                check(acc.get(), base.astype(np.float64) + want, C.TOL_ACT, what + " accumulate")
        if rows * cols > 100:
            assert not np.array_equal(P.dropout(x, keep, salt, 0), P.dropout(x, keep, salt, 1))
        same = Buf(dev, rows, cols, layout)
        ops.dropout(xd, same.view, 1.0, salt)
        check(same.get(), x, 0.0, "dropout keep_prob=1")


# ---- tanh_bwd ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.TANH_BWD_N)
def test_tanh_bwd(dev, n):
    """nm_tanh_bwd (in place, float4 body + scalar tail) for n < 4, n not a multiple of 4 and n past 2^20."""
    from neuralmonkey_amd import ops
    inp = C.tanh_bwd_inputs(n)
    want = C.tanh_bwd_expect(inp, np.float64)
    full, dy = _flat_guard(dev, n, init=inp["dy"])
    ops.tanh_bwd(dy, torch.tensor(inp["y"], device=dev))
    check(dy.cpu().numpy(), want, C.TOL_ACT, "tanh_bwd {}".format(n))
    assert _guards_intact(full)


# ---- embedding_scatter_add -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab,e,n,hot", C.SCATTER_CASES)
@pytest.mark.parametrize("skip_pad", [False, True])
def test_embedding_scatter_add(dev, vocab, e, n, hot, skip_pad):
    """nm_embedding_scatter_add: hundreds of rows onto the same few ids (the target side of a batch), id 0 present with
    skip_pad on and off, E not a multiple of 64, strided d, ids outside [0, V) ignored (the kernel checks the id before
    it forms an address), guard rows around the table intact.  Float atomics add in any order: the bound is that of a
    float32 sum of the row's addends."""
    from neuralmonkey_amd import ops
    ids, d, base = C.scatter_inputs(vocab, e, n, hot)
    want = P.embedding_grads(vocab, ids, torch.tensor(d, dtype=torch.float64), skip_pad).numpy()
    ok = C.scatter_kept(ids, vocab, skip_pad)
    direct = np.zeros((vocab, e))
    np.add.at(direct, ids[ok], d[ok].astype(np.float64))         # the restatement against np.add.at
    assert np.allclose(want, direct, rtol=0, atol=1e-12)
    counts = np.bincount(ids[ok], minlength=vocab)
    for layout in LAYOUTS:
        table = torch.tensor(base, device=dev)
        ops.embedding_scatter_add(table[1:vocab + 1], i32(dev, ids), dev_in(dev, d, layout), skip_pad=skip_pad)
        got = table.cpu().numpy()
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[-1], base[-1]), "guard rows written"
        err = np.abs(got[1:-1].astype(np.float64) - (base[1:-1] + want)).max(1)
        bnd = np.array([C.sum_bound(c + 1, float(np.abs(d).max())) for c in counts])
        print("scatter_add V={} E={} n={} {}: worst err/bound {:.3g}".format(vocab, e, n, layout, (err / bnd).max()))
        assert (err <= bnd).all()
        assert np.array_equal(got[1:-1][counts == 0], base[1:-1][counts == 0])       # untouched rows bit for bit


# ---- layer_norm_bwd ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,d", C.LN_SHAPES)
def test_layer_norm_bwd(dev, rows, d):
    """nm_layer_norm_bwd (the call encoders/recurrent.py and the tape still make): dx against autograd, dyx against
    dy * xhat, the column sums of dyx against dgamma."""
    from neuralmonkey_amd import ops
    inp = C.ln_inputs(rows, d)
    want = C.ln_expect(inp, np.float64)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=dev)
    fdx, dx = _flat_guard(dev, rows * d)
    fdyx, dyx = _flat_guard(dev, rows * d)
    ops.layer_norm_bwd(t(inp["dy"]), t(inp["x"]), t(C.np64(want["mean"])), t(C.np64(want["rstd"])), t(inp["gamma"]),
                       dx.view(rows, d), dyx.view(rows, d))
    check(dx.view(rows, d).cpu().numpy(), want["dx"], C.TOL_FUSED, "layer_norm_bwd {}x{} dx".format(rows, d))
    got_dyx = dyx.view(rows, d).cpu().numpy()
    check(got_dyx, want["dyx"], C.TOL_FUSED, "layer_norm_bwd {}x{} dyx".format(rows, d))
    dgamma = C.np64(want["dgamma"])
    assert np.abs(got_dyx.astype(np.float64).sum(0) - dgamma).max() <= C.bound(C.TOL_FUSED, dgamma) * np.sqrt(rows)
    assert _guards_intact(fdx) and _guards_intact(fdyx)


# ---- masked softmax pair -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", C.SOFTMAX_S)
@pytest.mark.parametrize("rpk", [1, 5])
def test_attn_softmax_fwd_bwd(dev, s, rpk):
    """nm_attn_softmax_fwd / _bwd: S on either side of the one-wave width, energies spread over +-40, B = 3 sentences
    with different masks (one fully masked: zero weights, finite gradient), T = 2; the forward takes mask row
    (r / rows_per_key) % B, the backward row % B; mask=None."""
    from neuralmonkey_amd import ops
    inp = C.softmax_inputs(s, rpk)
    rows = inp["e"].shape[0]
    for masked in (True, False):
        want = C.softmax_expect(inp, rpk, np.float64, masked)
        e, dw = torch.tensor(inp["e"], device=dev), torch.tensor(inp["dw"], device=dev)
        mask = torch.tensor(inp["mask"], device=dev) if masked else None
        fw, w = _flat_guard(dev, rows * s)
        ops.attn_softmax_fwd(e, mask, w.view(rows, s), C.SOFTMAX_B, rows_per_key=rpk)
        what = "attn_softmax S={} rpk={} masked={}".format(s, rpk, masked)
        got_w = w.view(rows, s).cpu().numpy()
        check(got_w, want["w"], C.TOL_FUSED, what + " w")
        fde, de = _flat_guard(dev, rows * s)
        ops.attn_softmax_bwd(dw, e, mask, de.view(rows, s), C.SOFTMAX_B)
        got_de = de.view(rows, s).cpu().numpy()
        check(got_de, want["de"], C.TOL_FUSED, what + " de")
        assert _guards_intact(fw) and _guards_intact(fde) and np.isfinite(got_de).all()
        if masked:
            dead_fwd = ((np.arange(rows) // rpk) % C.SOFTMAX_B) == 1
            assert np.array_equal(got_w[dead_fwd], np.zeros_like(got_w[dead_fwd]))
            assert np.abs(got_de[(np.arange(rows) % C.SOFTMAX_B) == 1]).max() == 0.0


# ---- Transformer utilities -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,t,d,t0", [(2, 3, 5, 2), (37, 1, 7, 0), (13, 50, 1617, 3), (6400, 1, 512, 0)])
def test_add_position(dev, b, t, d, t0):
    """nm_add_position with t0 > 0 and in the single-row form (T = 1, a [1, D] signal: the broadcast add of a target
    modality embedding); one add per element: bit for bit."""
    from neuralmonkey_amd import ops
    rng = np.random.default_rng([b, t, d])
    x, signal = C.normal(rng, (b, t, d)), C.normal(rng, (t0 + t, d))
    full, out = _flat_guard(dev, x.size)
    ops.add_position(torch.tensor(x, device=dev), torch.tensor(signal, device=dev), out.view(b, t, d), t0)
    assert np.array_equal(out.view(b, t, d).cpu().numpy(), P.add_position(x, signal, t0)) and _guards_intact(full)


@pytest.mark.parametrize("b,t,d", C.TIME_SUM_SHAPES)
def test_time_sum_and_its_gradient(dev, b, t, d):
    """nm_time_sum (written onto NaN) against a float64 sum; nm_time_bcast_add accumulates onto a base: one add per
    element, bit for bit; T = 1 and T = 50."""
    from neuralmonkey_amd import ops
    x, dy, base = C.time_sum_inputs(b, t, d)
    full, out = _flat_guard(dev, b * d)
    ops.time_sum(torch.tensor(x, device=dev), out.view(b, d))
    err = np.abs(out.view(b, d).cpu().numpy() - P.time_sum(torch.tensor(x, dtype=torch.float64)).numpy()).max()
    assert err <= C.sum_bound(t, float(np.abs(x).max())) and _guards_intact(full)
    if t == 1:
        assert np.array_equal(out.view(b, d).cpu().numpy(), x[:, 0])
    grad = P.time_sum_grads((b, t, d), torch.tensor(dy)).numpy()
    full2, dx = _flat_guard(dev, x.size, init=base)
    ops.time_bcast_add(torch.tensor(dy, device=dev), dx.view(b, t, d))
    assert np.array_equal(dx.view(b, t, d).cpu().numpy(), base + grad) and _guards_intact(full2)


@pytest.mark.parametrize("n", [1, 7, 1000])
def test_unfinished_mask_into_a_strided_column(dev, n):
    from neuralmonkey_amd import ops
    rng = np.random.default_rng(n)
    fin = rng.integers(0, 3, n).astype(np.int32)                 # any non-zero word counts as finished
    fin[0] = 1 if n == 1 else 0
    table = torch.full((n, 5), NAN, device=dev)
    ops.unfinished_mask(i32(dev, fin), table[:, 2])
    got = table.cpu().numpy()
    assert np.array_equal(got[:, 2], P.unfinished_mask(fin)) and np.isnan(np.delete(got, 2, axis=1)).all()


@pytest.mark.parametrize("rows,width", [(1, 5), (37, 300), (301, 257), (1031, 1021), (70000, 3)])
def test_copy_cols_and_log_softmax_from_stats(dev, rows, width):
    """nm_copy_cols and nm_log_softmax with strided rows, widths that are no multiple of 256, one row -- and more rows
    than one grid dimension holds (70000 > 65535: the kernels walk the rows).  A copy, and two correctly-rounded
    subtractions with nothing to contract: bit for bit."""
    from neuralmonkey_amd import ops
    rng = np.random.default_rng([rows, width])
    x = C.normal(rng, (rows, width), 3.0)
    rmax = x.max(1)
    rlse = np.log(np.exp(x.astype(np.float64) - rmax[:, None]).sum(1)).astype(np.float32)
    for src_layout in LAYOUTS:
        for dst_layout in LAYOUTS:
            xd = dev_in(dev, x, src_layout)
            dst = Buf(dev, rows, width, dst_layout)
            ops.copy_cols(xd, dst.view)
            check(dst.get(), x, 0.0, "copy_cols {}x{} {}->{}".format(rows, width, src_layout, dst_layout))
            out = Buf(dev, rows, width, dst_layout)
            ops.log_softmax_from_stats(xd, torch.tensor(rmax, device=dev), torch.tensor(rlse, device=dev), out.view)
            check(out.get(), P.log_softmax_from_stats(x, rmax, rlse), 0.0,
                  "log_softmax {}x{} {}->{}".format(rows, width, src_layout, dst_layout))


# ---- reduce_sum ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.REDUCE_N)
def test_reduce_sum_both_kernels(dev, n):
    """nm_reduce_sum on either side of the switch to the two-stage kernel (n > 65536), at the attention-bias gradient of
    the headline size (320 000) and at 65 537, where the last of the 64 slices is the shortest it can be (962 of 1025
    elements; it cannot be empty: that needs n <= 63 * 63, far below the switch).  Deterministic from launch to launch."""
    from neuralmonkey_amd import ops
    x = C.reduce_inputs(n)
    xd = torch.tensor(x, device=dev)
    out = torch.full((3,), NAN, device=dev)
    ops.reduce_sum(xd, out[1:2])
    got = out.cpu().numpy()
    assert np.isnan(got[0]) and np.isnan(got[2])
    assert abs(float(got[1]) - x.astype(np.float64).sum()) <= C.sum_bound(n, float(np.abs(x).max()))
    again = torch.full((1,), NAN, device=dev)
    ops.reduce_sum(xd, again)
    assert float(again[0]) == float(got[1])
    if n > 1:                                       # every slice is read: moving weight between the ends changes nothing else
        y = x.copy()
        y[0] += 1024.0
        ops.reduce_sum(torch.tensor(y, device=dev), again)
        assert abs(float(again[0]) - y.astype(np.float64).sum()) <= C.sum_bound(n, 1024.0)


# ---- greedy_update -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 300, 1000])
def test_greedy_update(dev, n):
    """nm_greedy_update against the restated decoder loop body: integer outputs exact, rows that were finished already
    emit 0 and stay finished, the all_finished word is cleared iff a row is still running; mask_out optional."""
    from neuralmonkey_amd import ops
    end = 2
    rng = np.random.default_rng(n)
    for everyone_ends in (False, True):
        argmax = rng.integers(0, 9, n).astype(np.int32)
        finished = (rng.random(n) < 0.3).astype(np.int32)
        if everyone_ends:
            argmax[finished == 0] = end
        else:
            argmax[0], finished[0] = 5, 0
        sym, fin, mask, allf = P.greedy_update(argmax, finished, end)
        assert allf == everyone_ends
        find, word = i32(dev, finished), i32(dev, [1])
        symd, maskd = torch.full((n + 2,), -77, dtype=torch.int32, device=dev), torch.full((n + 2,), -77, dtype=torch.int32, device=dev)
        ops.greedy_update(i32(dev, argmax), find, symd[1:n + 1], maskd[1:n + 1], end, all_finished=word)
        assert np.array_equal(symd.cpu().numpy(), np.concatenate([[-77], sym, [-77]]))
        assert np.array_equal(maskd.cpu().numpy(), np.concatenate([[-77], mask, [-77]]))
        assert np.array_equal(find.cpu().numpy(), fin) and int(word[0]) == int(allf)
        find2, sym2 = i32(dev, finished), torch.empty(n, dtype=torch.int32, device=dev)
        ops.greedy_update(i32(dev, argmax), find2, sym2, None, end)
        assert np.array_equal(sym2.cpu().numpy(), sym) and np.array_equal(find2.cpu().numpy(), fin)


# ---- gemm_group ----------------------------------------------------------------------------------------------------
def _group_case(dev, members, n, k, ta, tb, acc, what):
    from neuralmonkey_amd import ops
    items, refs, fulls = [], [], []
    for a_full, b_full, c0, a_np, b_np in members:
        out_full = torch.tensor(c0 if acc else np.full_like(c0, np.nan), device=dev)
        ref = P.gemm(a_np.astype(np.float64), b_np.astype(np.float64), ta, tb)
        refs.append(ref + c0[:, :n] if acc else ref)
        fulls.append((out_full, c0))
        items.append((torch.tensor(a_full, device=dev)[:, :a_np.shape[1]], torch.tensor(b_full, device=dev)[:, :b_np.shape[1]],
                      out_full[:, :n]))
    ops.gemm_group(items, trans_a=ta, trans_b=tb, accumulate=acc)
    for i, ((out_full, c0), ref) in enumerate(zip(fulls, refs)):             # every member, not just the first
        got = out_full.cpu().numpy()
        rel = np.abs(got[:, :n] - ref).max() / max(np.abs(ref).max(), 1e-6)
        assert rel < C.group_bound(k), "{} member {}: rel err {:.3g}".format(what, i, rel)
        if c0.shape[1] > n:
            assert np.array_equal(got[:, n:], c0[:, n:], equal_nan=True) if acc else np.isnan(got[:, n:]).all(), what


def _blocks128(m, n, count):
    return -(-m // 128) * -(-n // 128) * count


@pytest.mark.parametrize("m,n,k,ta,tb,count", C.GROUP_HAND)
def test_gemm_group_hand_picked(dev, m, n, k, ta, tb, count):
    """nm_gemm_f32_group at hand-picked shapes: 128x128 tiles (blocks128 >= 192) and 64x64 tiles in all four transpose
    combinations, the boundary itself (47 / 48 members of 2 x 2 tiles), deep K; contiguous and padded leading dimensions;
    accumulate off (NaN-filled outputs fully overwritten) and on; every member against float64."""
    for pads, acc, members in C.group_hand_runs(m, n, k, ta, tb, count):
        what = "m={} n={} k={} ta={} tb={} count={} pads={} acc={} big={}".format(
            m, n, k, ta, tb, count, pads, acc, _blocks128(m, n, count) >= 192)
        _group_case(dev, members, n, k, ta, tb, acc, what)


def test_gemm_group_random_shapes(dev):
    """nm_gemm_f32_group (the deferred weight gradients of every taped model, the highway products): a seeded sweep over
    the four transpose combinations, counts 1 / 2 / 6 / 48, ragged free extents (the contiguous ones are multiples of 4,
    as the header requires), leading dimensions wider than the rows, accumulate off and on -- every member against
    float64, bound 2e-6 sqrt(K) + 1e-6 relative as test_gemm."""
    seen = set()
    for what, (m, n, k, ta, tb, count), pads, acc, members in C.group_sweep_runs():
        seen.add((ta, tb))
        _group_case(dev, members, n, k, ta, tb, acc, what)
    assert len(seen) == 4


def test_gemm_group_transpose_detecting(dev):
    """A_i = I with asymmetric B_i (different for every member) catches a swapped C layout and a member written to
    another member's output, in both tile dispatches and all four layouts."""
    from neuralmonkey_amd import ops
    for n, count in ((96, 3), (256, 48)):
        assert (_blocks128(n, n, count) >= 192) == (count == 48)
        eye = np.eye(n, dtype=np.float32)
        bs = [((np.arange(n * n, dtype=np.float32).reshape(n, n) + 7 * i) % 97) * 0.25 for i in range(count)]
        for ta in (False, True):
            for tb in (False, True):
                items = [(torch.tensor(eye, device=dev), torch.tensor(np.ascontiguousarray(b.T) if tb else b, device=dev),
                          torch.full((n, n), NAN, device=dev)) for b in bs]
                ops.gemm_group(items, trans_a=ta, trans_b=tb, accumulate=False)
                for (_, _, out), b in zip(items, bs):
                    assert np.array_equal(out.cpu().numpy(), b), (n, count, ta, tb)


# ---- entry points that had no direct test of their own ----------------------------------------------------------------
def test_stream_read_yardstick_sums_what_it_reads(dev):
    """nm_prof_stream_read leaves one partial sum per workgroup in the sink: together they are the sum of the buffer
    (every float4 is read exactly once), below and above the 2048-workgroup cap."""
    from neuralmonkey_amd import _lib, ops
    lib = _lib.load()
    for n in (4, 1000 * 4, 2048 * 256 * 4 * 3 + 1028):
        rng = np.random.default_rng(n)
        x = C.normal(rng, (n,))
        blocks = min(2048, (n // 4 + 255) // 256)
        sink = torch.full((blocks + 2,), NAN, device=dev)
        _lib.check(lib.nm_prof_stream_read(ops._stream(), torch.tensor(x, device=dev).data_ptr(), n * 4,     # pylint: disable=protected-access
                                           sink[1:].data_ptr()), "nm_prof_stream_read")
        got = sink.cpu().numpy()
        assert np.isnan(got[0]) and np.isnan(got[-1]) and np.isfinite(got[1:-1]).all()
        assert abs(got[1:-1].astype(np.float64).sum() - x.astype(np.float64).sum()) <= C.sum_bound(n, float(np.abs(x).max()))


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_bf16x3_costing_product(dev, variant):
    """nm_gemm_bf16x3_nt (costing only): C = A . B^T with each fp32 operand as bf16 hi + lo.  hi + lo carries 16
    significant bits (residual <= 2^-17 |x|), the dropped lo . lo term is <= 2^-18 |a b|: a term is off by at most
    ~2^-15.4 |a b| and K of them add up like a random walk -> 2^-15 sqrt(K) max|a| max|b|.  One term (plain bf16):
    2^-8 relative per operand, 2^-7 sqrt(K) max|a| max|b|.  Whole tiles only (a costing kernel)."""
    from neuralmonkey_amd import _lib, ops
    lib = _lib.load()
    m, n, k = 256, 384, 512
    rng = np.random.default_rng(variant)
    a, b = C.normal(rng, (m, k)), C.normal(rng, (n, k), 0.05)
    want = a.astype(np.float64) @ b.astype(np.float64).T
    ad, bd = torch.tensor(a, device=dev), torch.tensor(b, device=dev)
    for terms, eps in ((3, 2.0 ** -15), (1, 2.0 ** -7)):
        out = torch.full((m, n + 4), NAN, device=dev)
        _lib.check(lib.nm_gemm_bf16x3_nt(ops._stream(), m, n, k, ad.data_ptr(), k, bd.data_ptr(), k, out.data_ptr(),    # pylint: disable=protected-access
                                         n + 4, terms, variant), "nm_gemm_bf16x3_nt")
        got = out.cpu().numpy()
        err = np.abs(got[:, :n] - want).max()
        print("bf16x3 variant {} terms {}: err {:.3g}".format(variant, terms, err))
        assert err <= eps * np.sqrt(k) * np.abs(a).max() * np.abs(b).max() and np.isnan(got[:, n:]).all()


class _Spec:
    def __init__(self, size, offset):
        self.size, self.offset = size, offset


W_A_CUT = (1001,)     # a shard's cut inside w_a: chunks of 1001 (a 1-element tail), 65536 and 3464, the last two at odd offsets


def _optimizer_setup(dev, seed, cuts=(), small=False):
    """A flat parameter buffer of four variables (one longer than a chunk, padded offsets) and its tables, cut at the
    flat offsets ``cuts`` as well; ``small``: without the long variable."""
    from collections import OrderedDict
    from types import SimpleNamespace
    from neuralmonkey_amd import ops
    sizes = OrderedDict([("w_a", 70001), ("bias_b", 37), ("frozen", 500), ("w_c", 1031)][1 if small else 0:])
    specs, off = OrderedDict(), 0
    for name, size in sizes.items():
        specs[name] = _Spec(size, off)
        off += (size + 3) // 4 * 4
    store = SimpleNamespace(specs=specs, device=dev)
    tables = ops.OptimizerTables(store, regularizable={"w_a", "frozen", "w_c"}, trainable={"w_a", "bias_b", "w_c"},
                                 cuts=cuts)
    rng = np.random.default_rng(seed)
    flat = lambda scale, positive=False: (np.abs(rng.standard_normal(off)) if positive else rng.standard_normal(off)) \
        .astype(np.float32) * np.float32(scale)
    return specs, tables, dict(theta=flat(0.3), grad=flat(0.05), s0=flat(0.01), s1=flat(1e-3, True))


def _optimizer_reference(specs, host, kind, l1w, l2w, clip, params):
    """float64: regulariser terms into the gradient (non-bias variables), per-tensor clip_by_norm, Adam / Adadelta on
    the trainable ones (oracle/torch_ref.py)."""
    from oracle import torch_ref as TR
    view = lambda buf, sp: torch.tensor(buf[sp.offset:sp.offset + sp.size], dtype=torch.float64)
    p, g, s0, s1 = ({n: view(host[k], sp) for n, sp in specs.items()} for k in ("theta", "grad", "s0", "s1"))
    reg = [n for n in ("w_a", "frozen", "w_c") if n in specs]
    for n in reg:
        g[n] = g[n] + l1w * torch.sign(p[n]) + 2.0 * l2w * p[n]
    l1 = sum(float(p[n].abs().sum()) for n in reg)
    l2 = sum(float((p[n] ** 2).sum()) for n in reg)
    train = [n for n in ("w_a", "bias_b", "w_c") if n in specs]
    sub = lambda d: {n: d[n] for n in train}
    pt, s0t, s1t = sub(p), sub(s0), sub(s1)
    if kind == 0:
        lr_t, b1, b2, eps = params
        for n in train:
            gg = g[n] * (clip / max(float(g[n].norm()), clip)) if clip else g[n]
            s0t[n] = b1 * s0t[n] + (1 - b1) * gg
            s1t[n] = b2 * s1t[n] + (1 - b2) * gg * gg
            pt[n] = pt[n] - lr_t * s0t[n] / (s1t[n].sqrt() + eps)
    else:
        lr, rho, eps = params[:3]
        TR.clip_and_adadelta(pt, sub(g), s0t, s1t, clip, lr=lr, rho=rho, eps=eps)
    p.update(pt), s0.update(s0t), s1.update(s1t)
    return p, g, s0, s1, (l1, l2)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("path", ["whole", "ranges", "lists", "whole-cut"])
def test_optimizer_kernels_direct(dev, kind, path):
    """The flat optimizer kernels called directly: nm_optim_regularize_norms + nm_optim_clip_adam / _clip_adadelta
    (one call each), nm_optim_partials + _segments + _apply over two chunk ranges, and the _list forms over a shuffled
    chunk list -- regularised gradient, L1 / L2, both slots and the parameters against float64; frozen and padding
    elements untouched.  ``whole-cut``: the first once more over a table cut inside w_a (``W_A_CUT``), whose chunks at
    odd element offsets run the kernels' scalar loops from end to end."""
    from neuralmonkey_amd import _lib, ops
    lib = _lib.load()
    specs, tables, host = _optimizer_setup(dev, 11 + kind, cuts=W_A_CUT if path == "whole-cut" else ())
    assert tables.nchunk == (6 if path == "whole-cut" else 5)
    if kind == 1:
        host["s0"] = np.abs(host["s0"])             # Adadelta's accumulators are sums of squares
    l1w, l2w, clip = 1e-3, 1e-2, 1.0
    params = (1e-3, 0.9, 0.999, 1e-8) if kind == 0 else (0.5, 0.95, 1e-6, 0.0)
    d = {k: torch.tensor(v, device=dev) for k, v in host.items()}
    if path.startswith("whole"):
        l1l2 = tables.regularize_and_norms(d["theta"], d["grad"], l1w, l2w)
        fn = lib.nm_optim_clip_adam if kind == 0 else lib.nm_optim_clip_adadelta
        args = params if kind == 0 else params[:3]
        _lib.check(fn(ops._stream(), d["theta"].data_ptr(), d["grad"].data_ptr(), d["s0"].data_ptr(),      # pylint: disable=protected-access
                      d["s1"].data_ptr(), *tables._tabs(), clip, *args, tables.workspace.data_ptr(),      # pylint: disable=protected-access
                      tables.workspace.numel() * 4), "nm_optim_clip_*")
    elif path == "ranges":
        cut = tables.nchunk // 2
        for rng_ in ((cut, tables.nchunk), (0, cut)):
            tables.partials(d["theta"], d["grad"], l1w, l2w, rng_)
        l1l2 = tables.segments()
        for rng_ in ((0, cut), (cut, tables.nchunk)):
            tables.apply(kind, d["theta"], d["grad"], d["s0"], d["s1"], clip, params, chunks=rng_)
    else:
        order = np.random.default_rng(3).permutation(tables.nchunk).astype(np.int32)
        lst = i32(dev, order)
        tables.partials(d["theta"], d["grad"], l1w, l2w, None, chunk_list=lst)
        l1l2 = tables.segments()
        tables.apply(kind, d["theta"], d["grad"], d["s0"], d["s1"], clip, params, chunk_list=lst)
    p, g, s0, s1, (l1, l2) = _optimizer_reference(specs, host, kind, l1w, l2w, clip, params)
    got_l = l1l2.cpu().numpy().astype(np.float64)
    # sums of positive terms, 256 of a chunk per thread one after the other: 2e-6 sqrt(256) of the sum itself
    assert abs(got_l[0] - l1) <= C.sum_bound(256, l1) and abs(got_l[1] - l2) <= C.sum_bound(256, l2)
    got = {k: v.cpu().numpy() for k, v in d.items()}
    covered = np.zeros(got["theta"].size, dtype=bool)
    for n, sp in specs.items():
        sl = slice(sp.offset, sp.offset + sp.size)
        covered[sl] = True
        for key, ref in (("theta", p), ("grad", g), ("s0", s0), ("s1", s1)):
            want = C.np64(ref[n])                   # 2e-5 of the tensor's largest entry (slots are ~1e-3: no max(1, .))
            err = np.abs(got[key][sl] - want).max()
            assert err <= 2e-5 * np.abs(want).max(), "optimizer kind {} {} {} {}: {:.3g}".format(kind, path, n, key, err)
        if n == "frozen":
            assert all(np.array_equal(got[key][sl], host[key][sl]) for key in ("theta", "s0", "s1"))
    assert all(np.array_equal(got[key][~covered], host[key][~covered]) for key in got)


@pytest.mark.parametrize("variant", ["sgd", "momentum", "adam"])
def test_optimizer_kernels_on_buffers_off_16_bytes(dev, variant):
    """One kind per slot count (none, one, two) over buffers that are 4-byte but not 16-byte aligned: every device buffer
    is the [1:] view of one an element longer.  The variables are the small ones, whose chunks all start on a multiple
    of four elements, so it is the buffers' addresses alone that must keep passes 1 and 3 off their float4 rows.  One
    update against float64 within 2e-5 x the tensor's largest entry; the frozen variable, the padding, the slots the
    kind lacks and the element in front of every buffer bit-unchanged."""
    from tests import optim_family_cases as OC
    keys = ("theta", "grad", "s0", "s1")
    specs, tables, host = _optimizer_setup(dev, 41, small=True)
    assert "w_a" not in specs and tables.nchunk == 3
    if variant == "adam":
        kind, slots, params = 0, 2, (1e-3, 0.9, 0.999, 1e-8)
        refs = _optimizer_reference(specs, host, kind, OC.L1W, OC.L2W, OC.CLIP, params)[:4]
        want = {key: {n: C.np64(ref[n]) for n in specs} for key, ref in zip(keys, refs)}
    else:
        from tests import optim_ref as R
        kind, params = OC.VARIANTS[variant]
        slots = R.SLOTS[kind]
        flat = OC.expected(specs, OC.prepare(host, variant), variant)[0]
        want = {key: {n: flat[key][sp.offset:sp.offset + sp.size] for n, sp in specs.items()} for key in keys}
    full = {k: torch.full((host[k].size + 1,), NAN, device=dev) for k in keys}
    d = {k: v[1:] for k, v in full.items()}
    for k in keys:
        d[k].copy_(torch.tensor(host[k]))
    assert all(v.data_ptr() % 16 == 4 for v in d.values())
    tables.regularize_and_norms(d["theta"], d["grad"], OC.L1W, OC.L2W)
    tables.apply(kind, d["theta"], d["grad"], d["s0"] if slots >= 1 else None, d["s1"] if slots == 2 else None, OC.CLIP,
                 params)
    assert all(bool(torch.isnan(v[0])) for v in full.values())
    got = {k: v.cpu().numpy() for k, v in d.items()}
    covered = np.zeros(got["theta"].size, dtype=bool)
    for n, sp in specs.items():
        sl = slice(sp.offset, sp.offset + sp.size)
        covered[sl] = True
        for key in keys:
            err, bound = np.abs(got[key][sl] - want[key][n]).max(), 2e-5 * np.abs(want[key][n]).max()
            print("{} {} {}: err {:.3g} bound {:.3g}".format(variant, n, key, err, bound))
            assert err <= bound, (variant, n, key, err, bound)
        if n == "frozen":
            assert all(np.array_equal(got[key][sl], host[key][sl]) for key in ("theta", "s0", "s1"))
        else:
            assert not np.array_equal(got["theta"][sl], host["theta"][sl])
    assert not covered.all() and all(np.array_equal(got[key][~covered], host[key][~covered]) for key in keys)
    for key, has in (("s0", slots >= 1), ("s1", slots == 2)):
        assert has or np.array_equal(got[key], host[key])



# ---- the coverage ledger -------------------------------------------------------------------------------------------
# Every entry point of include/nmhip.h -> "tests/<file>::<test>" of a test whose source calls it (by its symbol or by
# the wrapper named after "via"), or ("no kernel", reason) for entry points that launch no arithmetic kernel.
HERE = "tests/test_pointwise_kernels_gpu.py::"
K = "tests/test_kernels_gpu.py::"
ABI = "tests/test_abi.py::"
BEAM = "tests/test_beam_kernels_gpu.py::"      # float64 restatement of the beam body (oracle/beam_ref.py)
LEDGER = {
    # -- contexts, errors, profiler, communicator, test hooks, size queries: no arithmetic kernel
    "nm_last_error": ("no kernel", "thread-local error text"),
    "nm_version": ("no kernel", "a constant"),
    "nm_create": ("no kernel", "context plumbing"),
    "nm_destroy": ("no kernel", "context plumbing"),
    "nm_ctx_bind": ("no kernel", "context plumbing"),
    "nm_ctx_current": ("no kernel", "context plumbing"),
    "nm_ctx_device": ("no kernel", "context plumbing"),
    "nm_ctx_switch": ("no kernel", "context plumbing"),
    "nm_ctx_set_background": ("no kernel", "context plumbing: a launch-mode flag"),
    "nm_prof_enable": ("no kernel", "profiler plumbing"),
    "nm_prof_attn_step": ("no kernel", "profiler plumbing: reads event timers"),
    "nm_allreduce_unique_id": ("no kernel", "communicator plumbing"),
    "nm_allreduce_init": ("no kernel", "communicator plumbing"),
    "nm_allreduce_bucket": ("no kernel", "communicator plumbing: the sum is the collective library's"),
    "nm_allreduce_wait": ("no kernel", "communicator plumbing"),
    "nm_allreduce_destroy": ("no kernel", "communicator plumbing"),
    "nm_gru_seq_force_give_up": ("no kernel", "test hook: a host counter"),
    "nm_gru_seq_test_hog": ("no kernel", "test hook: sleeping workgroups"),
    "nm_gru_seq_failed": ("no kernel", "reads a workspace's error word"),
    "nm_gru_seq_supported": ("no kernel", "shape query"),
    "nm_dec_step_cluster_supported": ("no kernel", "shape query"),
    "nm_gru_seq_workspace_bytes": ("no kernel", "size query"),
    "nm_nematus_seq_workspace_bytes": ("no kernel", "size query"),
    "nm_lstm_seq_workspace_bytes": ("no kernel", "size query"),
    "nm_dec_step_cluster_workspace_bytes": ("no kernel", "size query"),
    "nm_attn_workspace_bytes": ("no kernel", "size query"),
    "nm_attn_partials_layout": ("no kernel", "layout query"),
    "nm_beam_workspace_bytes": ("no kernel", "size query"),
    "nm_colsum_workspace_bytes": ("no kernel", "size query"),
    "nm_layer_norm_bwd_params_workspace_bytes": ("no kernel", "size query"),
    "nm_logits_stats_tile": ("no kernel", "size query"),
    "nm_logits_stats_bytes": ("no kernel", "size query"),
    "nm_optim_workspace_bytes": ("no kernel", "size query"),
    "nm_proj_split_bytes": ("no kernel", "size query"),
    "nm_proj_split_forget": ("no kernel", "forgets a registration (host table)"),
    "nm_conv1d_wgrad_workspace_bytes": ("no kernel", "size query"),
    "nm_copy_d2d": ("no kernel", "a runtime device-to-device copy"),
    # -- this module
    "nm_ew": HERE + "test_ew_every_op_code via ops.ew",
    "nm_lstm_cell_fwd": HERE + "test_lstm_cell_fwd_bwd via ops.lstm_cell_fwd",
    "nm_lstm_cell_bwd": HERE + "test_lstm_cell_fwd_bwd via ops.lstm_cell_bwd",
    "nm_nematus_cell_fwd": HERE + "test_nematus_cell_fwd_bwd via ops.nematus_cell_fwd",
    "nm_nematus_cell_bwd": HERE + "test_nematus_cell_fwd_bwd via ops.nematus_cell_bwd",
    "nm_blend_fwd": HERE + "test_blend_fwd_bwd via ops.blend_fwd",
    "nm_blend_bwd": HERE + "test_blend_fwd_bwd via ops.blend_bwd",
    "nm_rnn_select_fwd": HERE + "test_rnn_select_fwd_bwd via ops.rnn_select_fwd",
    "nm_rnn_select_bwd": HERE + "test_rnn_select_fwd_bwd via ops.rnn_select_bwd",
    "nm_reverse_sequence": HERE + "test_reverse_sequence via ops.reverse_sequence",
    "nm_maxout_fwd": HERE + "test_maxout_fwd_bwd via ops.maxout_fwd",
    "nm_maxout_bwd": HERE + "test_maxout_fwd_bwd via ops.maxout_bwd",
    "nm_dropout": HERE + "test_dropout_salt_step_accumulate via ops.dropout",
    "nm_tanh_bwd": HERE + "test_tanh_bwd via ops.tanh_bwd",
    "nm_embedding_scatter_add": HERE + "test_embedding_scatter_add via ops.embedding_scatter_add",
    "nm_layer_norm_bwd": HERE + "test_layer_norm_bwd via ops.layer_norm_bwd",
    "nm_attn_softmax_fwd": HERE + "test_attn_softmax_fwd_bwd via ops.attn_softmax_fwd",
    "nm_attn_softmax_bwd": HERE + "test_attn_softmax_fwd_bwd via ops.attn_softmax_bwd",
    "nm_add_position": HERE + "test_add_position via ops.add_position",
    "nm_time_sum": HERE + "test_time_sum_and_its_gradient via ops.time_sum",
    "nm_time_bcast_add": HERE + "test_time_sum_and_its_gradient via ops.time_bcast_add",
    "nm_unfinished_mask": HERE + "test_unfinished_mask_into_a_strided_column via ops.unfinished_mask",
    "nm_copy_cols": HERE + "test_copy_cols_and_log_softmax_from_stats via ops.copy_cols",
    "nm_log_softmax": HERE + "test_copy_cols_and_log_softmax_from_stats via ops.log_softmax_from_stats",
    "nm_reduce_sum": HERE + "test_reduce_sum_both_kernels via ops.reduce_sum",
    "nm_greedy_update": HERE + "test_greedy_update via ops.greedy_update",
    "nm_gemm_f32_group": HERE + "test_gemm_group_random_shapes via ops.gemm_group",
    "nm_prof_stream_read": HERE + "test_stream_read_yardstick_sums_what_it_reads",
    "nm_gemm_bf16x3_nt": HERE + "test_bf16x3_costing_product",
    "nm_optim_regularize_norms": HERE + "test_optimizer_kernels_direct via ops.OptimizerTables.regularize_and_norms",
    "nm_optim_clip_adam": HERE + "test_optimizer_kernels_direct",
    "nm_optim_clip_adadelta": HERE + "test_optimizer_kernels_direct",
    "nm_optim_partials": HERE + "test_optimizer_kernels_direct via ops.OptimizerTables.partials",
    "nm_optim_partials_list": HERE + "test_optimizer_kernels_direct via ops.OptimizerTables.partials",
    "nm_optim_segments": HERE + "test_optimizer_kernels_direct via ops.OptimizerTables.segments",
    "nm_optim_apply": HERE + "test_optimizer_kernels_direct via ops.OptimizerTables.apply",
    "nm_optim_apply_list": HERE + "test_optimizer_kernels_direct via ops.OptimizerTables.apply",
    # -- covered elsewhere already
    "nm_crc32c": "tests/test_tf_bundle.py::test_crc32c_known_answers via tf_bundle.crc32c",
    "nm_gemm_f32": K + "test_gemm_random_shapes via ops.gemm",
    "nm_gemm_f32_chain": K + "test_chained_weight_and_bias_gradients via ops.gemm_chain",
    "nm_colsum_chain": K + "test_chained_weight_and_bias_gradients via ops.colsum_chain",
    "nm_outer_chain": K + "test_outer_products_of_a_loop_summed_in_one_launch via ops.outer_chain",
    "nm_embedding_gather": K + "test_embedding_gather via ops.embedding_gather",
    "nm_gru_gates_fwd": K + "test_gru_decoder_step via ops.gru_gates_fwd",
    "nm_gru_blend_fwd": K + "test_gru_decoder_step via ops.gru_blend_fwd",
    "nm_gru_gemm": K + "test_gru_gemm_fused_epilogues_fwd_bwd via gru.step_fwd",
    "nm_gru_seq_shift": K + "test_gru_gemm_fused_epilogues_fwd_bwd via ops.gru_seq_shift",
    "nm_gru_rh_seq": K + "test_gru_gemm_fused_epilogues_fwd_bwd via ops.gru_rh_seq",
    "nm_add_layer_norm_fwd": K + "test_add_layer_norm_is_add_then_layer_norm via ops.add_layer_norm_fwd",
    "nm_add_layer_norm_stats_fwd": K + "test_layer_norm_forward_kernels via ops.add_layer_norm_stats_fwd",
    "nm_layer_norm_fwd": K + "test_layer_norm_forward_kernels via ops.layer_norm_fwd",
    "nm_layer_norm_bwd_params": K + "test_layer_norm_bwd_with_parameter_gradients via ops.layer_norm_bwd_params",
    "nm_attn_fwd": K + "test_attention_fwd via ops.attn_fwd",
    "nm_attn_fwd_multi": K + "test_attention_time_major_all_steps via ops.attn_fwd_time_major",
    "nm_row_stats": K + "test_row_stats_and_argmax_ties via ops.row_stats",
    "nm_xent": K + "test_xent_fwd_and_grad via ops.xent",
    "nm_xent_colsum": K + "test_xent_with_column_sums via ops.xent_colsum",
    "nm_beam_topk_step": BEAM + "test_step_against_float64 via ops.beam_topk_step",
    "nm_gather_rows_f32": K + "test_gather_and_token_reorder via ops.gather_rows",
    "nm_beam_reorder_tokens": K + "test_gather_and_token_reorder via ops.beam_reorder_tokens",
    "nm_colsum": K + "test_colsum_both_kernels via ops.colsum",
    "nm_colsum_algo": K + "test_colsum_both_kernels via ops.colsum",
    "nm_test_xcc_ids": K + "test_workgroups_are_dealt_round_robin_to_the_xcds",
    "nm_gru_step_bwd": K + "test_gru_gemm_fused_epilogues_fwd_bwd via gru.bptt",
    "nm_attn_energy_bwd": "tests/test_attn_bwd_gpu.py::test_attn_energy_bwd_matches_torch via ops.attn_energy_bwd",
    "nm_attn_step_bwd": "tests/test_attn_bwd_gpu.py::test_attn_step_bwd_matches_float64_autograd via ops.attn_step_bwd",
    "nm_attn_fwd_partials": "tests/test_step_group_gpu.py::test_partials_merged_in_the_operand_loader via ops.attn_fwd_partials",
    "nm_step_group": "tests/test_step_group_gpu.py::test_plain_problems_share_a_launch via ops.StepGroup",
    # (a shape query that launches nothing -- but a test calls it for every case of the sweep, so it names that test)
    "nm_step_group_plan": "tests/test_step_group_sweep_gpu.py::test_sweep_case via ops.StepGroup",
    "nm_decoder_step_fused": "tests/test_step_group_gpu.py::test_decoder_step_fused_is_the_oracle_step via ops.DecoderStepCall",
    "nm_beam_backtrace": "tests/test_beam_fused_gpu.py::test_backtrace_equals_the_per_step_history_gather via ops.beam_backtrace",
    "nm_beam_topk_step_fused": BEAM + "test_step_against_float64 via ops.beam_topk_step_fused",
    "nm_beam_topk_step_tiles": BEAM + "test_step_against_float64 via ops.beam_topk_step_tiles",
    "nm_greedy_finish": "tests/test_logits_stats_gpu.py::test_greedy_finish_matches_the_reference_update via ops.greedy_finish",
    "nm_logits_stats_gemm": "tests/test_logits_stats_gpu.py::test_stats_gemm_logits_and_merged_statistics via ops.logits_stats_gemm",
    "nm_proj_split_prepare": "tests/test_proj_split_gpu.py::test_split_projection_against_float64_and_the_exact_kernel via ops.proj_split_prepare",
    "nm_conv1d_pool_fwd": "tests/test_sentence_cnn_gpu.py::test_conv_pool_forward_and_gradients_match_float64 via ops.conv1d_pool_fwd",
    "nm_conv1d_pool_bwd": "tests/test_sentence_cnn_gpu.py::test_conv_pool_forward_and_gradients_match_float64 via ops.conv1d_pool_bwd",
    "nm_highway_fwd": "tests/test_sentence_cnn_gpu.py::test_highway_layer_matches_float64 via autodiff.highway",
    "nm_highway_bwd": "tests/test_sentence_cnn_gpu.py::test_highway_layer_matches_float64 via autodiff.highway",
    "nm_gumbel_argmax": "tests/test_sampling_gpu.py::test_draw_equals_the_restated_gumbel_argmax via ops.gumbel_argmax",
    "nm_gru_seq_fwd": "tests/test_gru_cluster_gpu.py::test_forward_loop_in_one_launch_equals_the_stepwise_launches via ops.gru_seq_fwd",
    "nm_gru_seq_bwd": "tests/test_gru_cluster_gpu.py::test_bptt_loop_in_one_launch_equals_the_stepwise_launches via ops.gru_seq_bwd",
    "nm_nematus_seq_fwd": "tests/test_nematus_cluster_gpu.py::test_nematus_loops_against_the_oracle via ops.nematus_seq_fwd",
    "nm_nematus_seq_bwd": "tests/test_nematus_cluster_gpu.py::test_nematus_loops_against_the_oracle via ops.nematus_seq_bwd",
    "nm_lstm_seq_fwd": "tests/test_nematus_cluster_gpu.py::test_lstm_loops_against_float64 via ops.lstm_seq_fwd",
    "nm_lstm_seq_bwd": "tests/test_nematus_cluster_gpu.py::test_lstm_loops_against_float64 via ops.lstm_seq_bwd",
    "nm_nematus_state_step": "tests/test_nematus_state_step_gpu.py::test_state_step_matches_float64_and_the_two_launches via ops.nematus_state_step",
    "nm_nematus_full_step": "tests/test_nematus_state_step_gpu.py::test_full_step_matches_float64 via ops.nematus_full_step",
    "nm_sdp_attn_fwd": "tests/test_transformer_gpu.py::test_sdp_attention_fwd_bwd via ops.sdp_attn_fwd",
    "nm_sdp_attn_bwd": "tests/test_transformer_gpu.py::test_sdp_attention_fwd_bwd via ops.sdp_attn_bwd",
    "nm_sdp_attn_step": "tests/test_transformer_gpu.py::test_sdp_step_through_an_ancestor_table via ops.sdp_attn_step",
    "nm_zero_if": "tests/test_cluster_recovery_gpu.py::test_the_garbage_update_is_skipped_on_the_device via ops.zero_if",
    "nm_fill_u32": "tests/test_no_foreign_kernels_gpu.py::test_fill_and_copy_are_runtime_operations via ops.fill",
}
