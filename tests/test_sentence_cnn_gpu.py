"""SentenceCNNEncoder on the MI355X: the fused conv + bias + relu + segment-max kernels (MFMA and scalar) and the
highway kernels against float64 restatements (tests/conv1d_ref.py: the references, the slab plan of the weight gradient
and the fp32 summation bound of the tests in the middle of this file), and tests/small_sent_cnn.ini -- loaded byte for byte from its bundle --
training, decoding and surviving a save / load round trip."""
import math

import numpy as np
import pytest
import torch

from . import conv1d_ref as R
from .conv1d_ref import _ref_conv, _ref_conv_t, _ref_pool, _ref_wgrad
from .test_sentence_cnn import cnn_root  # noqa: F401  pylint: disable=unused-import

pytestmark = pytest.mark.gpu


CASES = [  # (B, S, E, [(w, n)], s, algo)
    (3, 10, 11, [(1, 13), (2, 13), (3, 13)], 5, 0),       # tests/small_sent_cnn.ini's encoder, S a multiple of s
    (3, 12, 11, [(1, 13), (2, 13), (3, 13)], 5, 0),       # S = 12, s = 5: the windows shift
    (2, 13, 11, [(2, 300), (5, 13)], 5, 0),
    (2, 53, 128, [(4, 200), (8, 300)], 5, 0),
    (2, 50, 128, [(1, 13), (3, 200), (5, 300)], 5, 0),
    (3, 7, 11, [(2, 13), (4, 200)], 3, 0),
    (2, 131, 128, [(3, 200)], 128, 0),                   # the widest window of the MFMA path
    (2, 29, 128, [(2, 13), (8, 200)], 4, 2),             # the scalar kernels on the same ground
    (2, 23, 11, [(9, 13), (1, 13)], 6, 0),               # a width the MFMA path does not take: scalar kernels
    (3, 12, 11, [(1, 13), (2, 13), (3, 13)], 5, 2),
    # more than one forward time tile (25 windows of 5) and more than one 128-row data-gradient tile, S mod 5 = 1 / 4 / 0
    (2, 126, 128, [(2, 200), (3, 13), (8, 300)], 5, 0),
    (2, 131, 11, [(1, 13), (4, 200), (5, 300)], 5, 0),
    (2, 250, 128, [(2, 13), (7, 300)], 5, 0),
    (2, 129, 128, [(6, 200), (1, 300)], 5, 0),
    (2, 126, 11, [(2, 13), (3, 200)], 5, 2),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B{}-S{}-E{}-{}-s{}-algo{}".format(
    c[0], c[1], c[2], "_".join("{}x{}".format(w, n) for w, n in c[3]), c[4], c[5]))
def test_conv_pool_forward_and_gradients_match_float64(dev, case):
    from neuralmonkey_amd import ops
    bsz, slen, e, filters, s, algo = case
    g = torch.Generator().manual_seed(7)
    x = torch.randn(bsz, slen, e, generator=g, dtype=torch.float64)
    ws = [torch.randn(w, e, n, generator=g, dtype=torch.float64) / math.sqrt(w * e) for w, n in filters]
    bs = [torch.randn(n, generator=g, dtype=torch.float64) * 0.1 for _, n in filters]
    width = sum(n for _, n in filters)
    sp, pb = ops.conv1d_pool_shape(slen, s)
    lengths = torch.randint(1, slen + 1, (bsz,), generator=g, dtype=torch.int32)
    lengths[0] = min(slen, s)                          # a sentence of one segment
    mask = (torch.arange(slen)[None, :] < lengths[:, None].long()).double()

    f32 = lambda t: t.float().contiguous().to(dev)
    xd, wd, bd = f32(x), [f32(w) for w in ws], [f32(b) for b in bs]
    pooled = torch.empty(bsz, sp, width, device=dev)
    arg = torch.empty(bsz, sp, width, dtype=torch.int32, device=dev)
    mask_out = torch.empty(bsz, sp, device=dev)
    lens_out = torch.empty(bsz, dtype=torch.int32, device=dev)
    ops.conv1d_pool_fwd(xd, wd, bd, s, pooled, arg, mask=f32(mask), lengths=lengths.to(dev), mask_out=mask_out,
                        seq_lens=lens_out, algo=algo)
    torch.cuda.synchronize()

    # forward: values within the fp32 error scale of the products, every argmax a (near-)maximum of its window
    convs = _ref_conv(x, ws, bs)
    scales = _ref_conv(x.abs(), [w.abs() for w in ws], [b.abs() for b in bs])
    ref = torch.cat([_ref_pool(torch.relu(c), s) for c in convs], 1).transpose(1, 2)           # [B, S', F]
    scale = torch.cat([_ref_pool(c, s) for c in scales], 1).transpose(1, 2)
    tol = 1e-6 * scale + 1e-7
    got = pooled.double().cpu()
    assert bool(((got - ref).abs() <= 10 * tol).all()), float((got - ref).abs().max())
    relu_all = torch.relu(torch.cat(convs, 1))                                                    # [B, F, S]
    a = arg.long().cpu()
    j = torch.arange(sp)[None, :, None]
    assert bool(((a >= j * s - pb) & (a < j * s - pb + s) & (a >= 0) & (a < slen)).all())
    at_arg = relu_all.gather(2, a.transpose(1, 2)).transpose(1, 2)
    assert bool(((at_arg - ref).abs() <= 10 * tol).all())
    # the pooled mask and lengths (mask can be one segment longer than ceil(len / s))
    assert torch.equal(mask_out.cpu().double(), _ref_pool(mask[:, None, :], s)[:, 0])
    assert torch.equal(lens_out.cpu(), (lengths + s - 1) // s)

    # backward: the gradient routed through the kernel's argmax (where pooled > 0), then float64 autograd
    dpooled = torch.randn(bsz, sp, width, generator=g, dtype=torch.float64)
    gate = got > 0
    dz = torch.zeros(bsz, slen, width, dtype=torch.float64)
    dz.scatter_add_(1, a, torch.where(gate, dpooled, torch.zeros_like(dpooled)))
    x64 = x.clone().requires_grad_(True)
    w64 = [w.clone().requires_grad_(True) for w in ws]
    b64 = [b.clone().requires_grad_(True) for b in bs]
    outs = _ref_conv(x64, w64, b64)
    col = 0
    for o, (_, n) in zip(outs, filters):
        o.backward(dz[:, :, col:col + n].transpose(1, 2))
        col += n
    dzd = torch.empty(bsz, slen, width, device=dev)
    dx = torch.full((bsz, slen, e), 0.5, device=dev)                 # accumulate onto 0.5
    dws = [torch.zeros_like(w) for w in wd]
    dbs = [torch.full_like(b, 0.25) for b in bd]                      # accumulate onto 0.25
    wsp = torch.empty(max(1, ops.conv1d_wgrad_workspace_floats(bsz, slen, e, wd)), device=dev)
    ops.conv1d_pool_bwd(xd, wd, s, pooled, arg, f32(dpooled), dzd, dx=dx, accumulate_dx=True, dweights=dws,
                        dbiases=dbs, accumulate_params=True, workspace=wsp, algo=algo)
    torch.cuda.synchronize()
    assert torch.equal(dzd.cpu().double(), dz.float().double())
    # error scales ~1e-6 sum |a b| of each product
    adz = dz.abs()
    sx = _ref_conv_t(adz, [w.abs() for w in ws], filters)
    assert bool(((dx.cpu().double() - 0.5 - x64.grad).abs() <= 1e-5 * sx + 1e-6).all())
    for i, (w, (width_i, n)) in enumerate(zip(w64, filters)):
        sw = _ref_wgrad(x.abs(), adz[:, :, sum(m for _, m in filters[:i]):][:, :, :n], width_i)
        assert bool(((dws[i].cpu().double() - w.grad).abs() <= 1e-5 * sw + 1e-6).all()), i
        assert bool(((dbs[i].cpu().double() - 0.25 - b64[i].grad).abs() <= 1e-5 * adz.sum((0, 1))[
            sum(m for _, m in filters[:i]):][:n] + 1e-6).all()), i
    # deterministic: a second run is bit-identical
    dws2 = [torch.zeros_like(w) for w in wd]
    dbs2 = [torch.full_like(b, 0.25) for b in bd]
    dx2 = torch.full((bsz, slen, e), 0.5, device=dev)
    ops.conv1d_pool_bwd(xd, wd, s, pooled, arg, f32(dpooled), dzd, dx=dx2, accumulate_dx=True, dweights=dws2,
                        dbiases=dbs2, accumulate_params=True, workspace=wsp, algo=algo)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx2) and all(torch.equal(p, q) for p, q in zip(dws + dbs, dws2 + dbs2))


# ---- the slab path of the weight gradient, strides, flags, segment edges and the tie rule -----------------------------
# Bounds: tests/conv1d_ref.py (gamma(K) times the same expression on the absolute values, K counted per quantity).
NAN = float("nan")
STARTS = (0.5, 0.125, 0.25)                       # what an accumulating run finds in dx, dW and db
SMALL_FILTERS = [(2, 13), (4, 70)]


class _Problem:
    """One shape's operands: float64 copies of the fp32 values on the host, the fp32 values on the device.  With ``pad``
    x and dx are [B, S, E] views of buffers filled with 7.0 whose rows lie E + pad floats apart."""

    def __init__(self, dev, bsz, slen, e, filters, s, seed, pad=0, inputs=None):
        from neuralmonkey_amd import ops
        self.dev, self.dims, self.filters, self.s, self.pad = dev, (bsz, slen, e), filters, s, pad
        self.x, self.ws, self.bs, g = inputs or R.pool_inputs(bsz, slen, e, filters, s, seed)
        self.width = sum(n for _, n in filters)
        self.sp, self.pb = ops.conv1d_pool_shape(slen, s)
        self.lengths = torch.randint(1, slen + 1, (bsz,), generator=g, dtype=torch.int32)
        self.lengths[0] = min(slen, s)                 # a sentence of one segment
        self.mask = (torch.arange(slen)[None, :] < self.lengths[:, None].long()).double()
        self.dpooled = torch.randn(bsz, self.sp, self.width, generator=g, dtype=torch.float64).float().double()
        assert bool((self.dpooled != 0).all())
        f32 = lambda t: t.float().contiguous().to(dev)
        self.x_full, self.xd = self.rows()
        self.xd.copy_(self.x.float())
        self.wd, self.bd = [f32(w) for w in self.ws], [f32(b) for b in self.bs]
        self.maskd, self.lengthsd, self.dpooledd = f32(self.mask), self.lengths.to(dev), f32(self.dpooled)
        self.plan = R.slab_plan(bsz, slen, e, filters)
        assert ops.conv1d_wgrad_workspace_floats(bsz, slen, e, self.wd) * 4 == self.plan["bytes"]
        self.fwd_ref = None

    def rows(self):
        bsz, slen, e = self.dims
        full = torch.full((bsz, slen, e + self.pad), 7.0, device=self.dev)
        return full, full[:, :, :e]

    def outputs(self):
        bsz = self.dims[0]
        return (torch.full((bsz, self.sp, self.width), NAN, device=self.dev),
                torch.full((bsz, self.sp, self.width), -1, dtype=torch.int32, device=self.dev),
                torch.full((bsz, self.sp), NAN, device=self.dev),
                torch.full((bsz,), -1, dtype=torch.int32, device=self.dev))

    def forward(self, algo=0):
        from neuralmonkey_amd import ops
        pooled, arg, mask_out, lens_out = self.outputs()
        ops.conv1d_pool_fwd(self.xd, self.wd, self.bd, self.s, pooled, arg, mask=self.maskd, lengths=self.lengthsd,
                            mask_out=mask_out, seq_lens=lens_out, algo=algo)
        torch.cuda.synchronize()
        return pooled, arg, mask_out, lens_out

    def forward_direct(self, mask=False, lengths=False, algo=0):
        """The entry point itself: the mask pair and the lengths pair each present or null."""
        from neuralmonkey_amd import _lib, ops
        bsz, slen, e = self.dims
        pooled, arg, mask_out, lens_out = self.outputs()
        widths, counts, wtab = ops._conv_tables(self.wd)
        rc = _lib.load().nm_conv1d_pool_fwd(
            ops._stream(), self.xd.data_ptr(), self.xd.stride(1), bsz, slen, e, self.s, len(self.wd), widths, counts,
            wtab, ops._ptrs(self.bd), pooled.data_ptr(), arg.data_ptr(), self.width,
            self.maskd.data_ptr() if mask else None, self.lengthsd.data_ptr() if lengths else None,
            mask_out.data_ptr() if mask else None, lens_out.data_ptr() if lengths else None, algo)
        _lib.check(rc, "nm_conv1d_pool_fwd")
        torch.cuda.synchronize()
        return pooled, arg, mask_out, lens_out

    def check_forward(self, fwd, label, quantity="pool pooled"):
        """pooled within the bound; every argmax inside its window and a maximum of it up to twice the bound (the kernel
        chose it by values that each lie within one bound of float64's); the pooled mask and lengths exact."""
        pooled, arg, mask_out, lens_out = fwd
        bsz, slen, e = self.dims
        if self.fwd_ref is None:
            self.fwd_ref = R.pool_forward_ref(self.x, self.ws, self.bs, self.s)
        ref, mag, relu_all = self.fwd_ref
        k = R.forward_k(e, self.filters)
        R.within(pooled, ref, k, mag, label + " pooled", quantity)
        a = arg.long().cpu()
        j = torch.arange(self.sp)[None, :, None]
        assert bool(((a >= j * self.s - self.pb) & (a < j * self.s - self.pb + self.s) & (a >= 0) & (a < slen)).all())
        at_arg = relu_all.gather(2, a.transpose(1, 2)).transpose(1, 2)
        assert bool(((at_arg - ref).abs() <= 2 * (R.gamma(k) * mag + k * R.TINY)).all()), label
        assert torch.equal(mask_out.cpu().double(), _ref_pool(self.mask[:, None, :], self.s)[:, 0])
        assert torch.equal(lens_out.cpu(), (self.lengths + self.s - 1) // self.s)

    def backward_ref(self, pooled, arg):
        """float64 gradients of the routing the device chose (its pooled > 0 gate, its argmax) and their magnitudes."""
        bsz, slen, e = self.dims
        gated = torch.where(pooled.double().cpu() > 0, self.dpooled, torch.zeros_like(self.dpooled))
        dz = torch.zeros(bsz, slen, self.width, dtype=torch.float64).scatter_add_(1, arg.long().cpu(), gated)
        assert bool((dz > 0).any()) and bool((dz < 0).any())
        adz, aws = dz.abs(), [w.abs() for w in self.ws]
        cols = [sum(n for _, n in self.filters[:i]) for i in range(len(self.filters))]
        return dict(
            dz=dz, dx=_ref_conv_t(dz, self.ws, self.filters), dx_mag=_ref_conv_t(adz, aws, self.filters),
            dw=[_ref_wgrad(self.x, dz[:, :, c:c + n], w) for c, (w, n) in zip(cols, self.filters)],
            dw_mag=[_ref_wgrad(self.x.abs(), adz[:, :, c:c + n], w) for c, (w, n) in zip(cols, self.filters)],
            db=[gated.sum((0, 1))[c:c + n] for c, (_, n) in zip(cols, self.filters)],
            db_mag=[gated.abs().sum((0, 1))[c:c + n] for c, (_, n) in zip(cols, self.filters)])

    def backward(self, pooled, arg, accumulate, algo=0, dx=True, params=True):
        """One call onto NaN (overwriting) or STARTS (accumulating); the workspace holds NaN."""
        from neuralmonkey_amd import ops
        bsz, slen, e = self.dims
        start = STARTS if accumulate else (NAN, NAN, NAN)
        dz = torch.full((bsz, slen, self.width), NAN, device=self.dev)
        dx_full, dxv = self.rows()
        dxv.fill_(start[0])
        dws = [torch.full_like(w, start[1]) for w in self.wd]
        dbs = [torch.full_like(b, start[2]) for b in self.bd]
        wsp = torch.full((self.plan["bytes"] // 4,), NAN, device=self.dev)
        ops.conv1d_pool_bwd(self.xd, self.wd, self.s, pooled, arg, self.dpooledd, dz, dx=dxv if dx else None,
                            accumulate_dx=accumulate, dweights=dws if params else None,
                            dbiases=dbs if params else None, accumulate_params=accumulate,
                            workspace=wsp if params else None, algo=algo)
        torch.cuda.synchronize()
        return dz, dx_full, dxv, dws, dbs

    def check_backward(self, out, ref, accumulate, label, tag=""):
        dz, dx_full, dxv, dws, dbs = out
        bsz, slen, e = self.dims
        assert torch.equal(dz.cpu().double(), ref["dz"]), label          # routed values, no arithmetic: exact
        acc = 1 if accumulate else 0
        start = STARTS if accumulate else (0.0, 0.0, 0.0)
        R.within(dxv, ref["dx"] + start[0], sum(w * n for w, n in self.filters) + acc, ref["dx_mag"] + start[0],
                 label + " dx", "pool dx" + tag)
        for i in range(len(self.filters)):
            R.within(dws[i], ref["dw"][i] + start[1], bsz * slen + self.plan["slices"] + acc,
                     ref["dw_mag"][i] + start[1], "{} dW_{}".format(label, i), "pool dW" + tag)
            R.within(dbs[i], ref["db"][i] + start[2], bsz * self.sp + 16 + acc, ref["db_mag"][i] + start[2],
                     "{} db_{}".format(label, i), "pool db" + tag)
        if self.pad:
            assert bool((dx_full[:, :, e:] == 7.0).all()) and bool((self.x_full[:, :, e:] == 7.0).all()), label

    def check_both_algos(self, label, gate_fraction=True):
        """Forward, then both backward modes, under the automatic choice and under the scalar kernels, against one
        float64 reference; returns the runs by algo."""
        runs = {}
        for algo, tag in ((0, ""), (2, " (scalar)")):
            fwd = self.forward(algo)
            self.check_forward(fwd, "{} algo {}".format(label, algo), "pool pooled" + tag)
            runs[algo] = fwd
        pooled, arg = runs[0][:2]
        positive = float((pooled > 0).float().mean())
        print("conv1d gate | {} | {:.3f} of pooled is positive".format(label, positive))
        if gate_fraction:
            assert 0.2 < positive < 0.8, positive                        # the relu gate matters
        ref = self.backward_ref(pooled, arg)
        for algo, tag in ((0, ""), (2, " (scalar)")):
            for accumulate in (False, True):
                out = self.backward(pooled, arg, accumulate, algo)
                self.check_backward(out, ref, accumulate, "{} algo {} acc {}".format(label, algo, int(accumulate)), tag)
                runs[algo, accumulate] = out
        again = self.backward(pooled, arg, True, 0)                      # fixed order: bit-equal
        assert all(torch.equal(p, q) for p, q in zip(_flat(runs[0, True]), _flat(again))), label
        return runs, ref


def _flat(out):
    dz, dx_full, _, dws, dbs = out
    return [dz, dx_full] + list(dws) + list(dbs)


@pytest.mark.parametrize("name", sorted(R.POOL_SLAB_CASES))
def test_weight_gradient_slabs_match_float64(dev, name):
    """P1-P6 of tests/conv1d_ref.py: two to 32 position slabs (P5: one, just below the threshold), segments of 5."""
    (bsz, slen, e, filters), _, slices, per, last = R.POOL_SLAB_CASES[name]
    p = _Problem(dev, bsz, slen, e, filters, 5, seed=100 + int(name[1:]))
    assert (p.plan["slices"], p.plan["per"], p.plan["last"]) == (slices, per, last)
    p.check_both_algos(name)


@pytest.mark.parametrize("algo", [0, 2])
def test_rows_of_x_and_dx_wider_than_e(dev, algo):
    """ldx = E + 3: dx shares x's stride; what lies between the rows keeps its 7.0."""
    p = _Problem(dev, 3, 37, 11, SMALL_FILTERS, 5, seed=21, pad=3)
    assert p.xd.stride(1) == 14 and not p.xd.is_contiguous()
    fwd = p.forward(algo)
    p.check_forward(fwd, "strided algo {}".format(algo), "pool pooled strided")
    ref = p.backward_ref(*fwd[:2])
    for accumulate in (False, True):
        out = p.backward(fwd[0], fwd[1], accumulate, algo)
        p.check_backward(out, ref, accumulate, "strided algo {} acc {}".format(algo, int(accumulate)), " strided")
    # the same values from contiguous rows, bit for bit
    q = _Problem(dev, 3, 37, 11, SMALL_FILTERS, 5, seed=21)
    fwd_q = q.forward(algo)
    assert torch.equal(fwd[0], fwd_q[0]) and torch.equal(fwd[1], fwd_q[1])
    out_q = q.backward(fwd_q[0], fwd_q[1], True, algo)
    assert torch.equal(out[2], out_q[2]) and all(torch.equal(a, b) for a, b in zip(out[3] + out[4], out_q[3] + out_q[4]))


@pytest.mark.parametrize("algo", [0, 2])
@pytest.mark.parametrize("accumulate", [False, True])
def test_dx_alone_and_parameters_alone_equal_the_full_call(dev, algo, accumulate):
    p = _Problem(dev, 3, 37, 11, SMALL_FILTERS, 5, seed=22)
    pooled, arg = p.forward(algo)[:2]
    dz, _, dx, dws, dbs = p.backward(pooled, arg, accumulate, algo)
    untouched = (lambda t, v: bool((t == v).all())) if accumulate else (lambda t, v: bool(torch.isnan(t).all()))
    dz1, _, dx1, dws1, dbs1 = p.backward(pooled, arg, accumulate, algo, dx=False)           # dx=None
    assert torch.equal(dz1, dz) and all(torch.equal(a, b) for a, b in zip(dws1 + dbs1, dws + dbs))
    assert untouched(dx1, STARTS[0])
    dz2, _, dx2, dws2, dbs2 = p.backward(pooled, arg, accumulate, algo, params=False)       # dweights=None
    assert torch.equal(dz2, dz) and torch.equal(dx2, dx)
    assert all(untouched(t, STARTS[1]) for t in dws2) and all(untouched(t, STARTS[2]) for t in dbs2)


@pytest.mark.parametrize("algo", [0, 2])
def test_forward_without_the_mask_or_the_lengths(dev, algo):
    p = _Problem(dev, 3, 37, 11, SMALL_FILTERS, 5, seed=23)
    pooled, arg, mask_out, lens_out = p.forward(algo)
    for mask, lengths in ((False, False), (True, False), (False, True), (True, True)):
        got = p.forward_direct(mask, lengths, algo)
        assert torch.equal(got[0], pooled) and torch.equal(got[1], arg), (mask, lengths)
        assert torch.equal(got[2], mask_out) if mask else bool(torch.isnan(got[2]).all())
        assert torch.equal(got[3], lens_out) if lengths else bool((got[3] == -1).all())


@pytest.mark.parametrize("slen,s,shape", [(37, 1, (37, 0)), (37, 40, (1, 1)), (140, 129, (2, 59))],
                         ids=["s1", "s-above-S", "s129"])
def test_segment_edges(dev, slen, s, shape):
    """Segments of one position, one window longer than the sentence (SAME pad in front), and 129 > 128 positions: the
    only route by segment size to the scalar kernels, where auto and algo=2 are the same launches."""
    bsz, e = 2, 11
    p = _Problem(dev, bsz, slen, e, SMALL_FILTERS, s, seed=24 + s)
    assert (p.sp, p.pb) == shape
    runs, ref = p.check_both_algos("s{}".format(s), gate_fraction=False)
    assert bool((runs[0][0] > 0).any()) and bool((runs[0][0] == 0).any())
    if s > 128:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[2]))
        for accumulate in (False, True):
            assert all(torch.equal(a, b) for a, b in zip(_flat(runs[0, accumulate]), _flat(runs[2, accumulate])))
        return
    _, mag, _ = p.fwd_ref
    R.within(runs[0][0], runs[2][0].double().cpu(), R.forward_k(e, SMALL_FILTERS), mag, "s{} auto vs scalar pooled".format(s),
             "pool auto vs scalar")
    for accumulate in (False, True):                                      # the same routing into both
        a, b = runs[0, accumulate], runs[2, accumulate]
        acc = int(accumulate)
        start = STARTS if accumulate else (0.0, 0.0, 0.0)
        R.within(a[2], b[2].double().cpu(), sum(w * n for w, n in SMALL_FILTERS) + acc, ref["dx_mag"] + start[0],
                 "s{} auto vs scalar dx".format(s), "pool auto vs scalar")
        for i in range(len(SMALL_FILTERS)):
            R.within(a[3][i], b[3][i].double().cpu(), bsz * slen + p.plan["slices"] + acc, ref["dw_mag"][i] + start[1],
                     "s{} auto vs scalar dW_{}".format(s, i), "pool auto vs scalar")
            assert torch.equal(a[4][i], b[4][i])                          # one bias kernel


@pytest.mark.parametrize("algo", [0, 2])
@pytest.mark.parametrize("slen,pb", [(12, 1), (10, 0)])
def test_ties_go_to_the_lowest_position(dev, slen, pb, algo):
    """Width-1 filters over a sentence that repeats its first position: every position of a window holds the same bits,
    and the argmax is the window's first valid position, max(0, j s - pb) -- tf.nn.max_pool's choice."""
    bsz, e, s, filters = 3, 11, 5, [(1, 13), (1, 70)]
    x, ws, bs, g = R.pool_inputs(bsz, slen, e, filters, 1, seed=41)      # (biases for windows of one: half positive)
    x = x[:, :1, :].expand(bsz, slen, e).contiguous()
    p = _Problem(dev, bsz, slen, e, filters, s, seed=None, inputs=(x, ws, bs, g))
    assert p.pb == pb
    pooled, arg, _, _ = fwd = p.forward(algo)
    p.check_forward(fwd, "ties S {} algo {}".format(slen, algo), "pool pooled ties")
    assert bool((pooled == pooled[:, :1, :]).all())
    first = (torch.arange(p.sp) * s - pb).clamp(min=0)
    assert torch.equal(arg.long().cpu(), first[None, :, None].expand(bsz, p.sp, p.width))
    gate = pooled.cpu() > 0
    assert 0.2 < float(gate.float().mean()) < 0.8
    dz = p.backward(pooled, arg, False, algo)[0].cpu().double()
    want = torch.zeros_like(dz)
    want[:, first, :] = torch.where(gate, p.dpooled, torch.zeros_like(p.dpooled))
    assert torch.equal(dz, want)
    nonzero = torch.zeros_like(dz, dtype=torch.bool)
    nonzero[:, first, :] = gate
    assert torch.equal(dz != 0, nonzero)


# ---- the highway kernels, called directly ------------------------------------------------------------------------------
def _padded2(rows, cols, pad, dev, values=None):
    """A [rows, cols] view (NaN, or ``values``) of a buffer of rows cols + pad floats long, filled with 7.0."""
    full = torch.full((rows, cols + pad), 7.0, device=dev)
    view = full[:, :cols]
    if values is None:
        view.fill_(NAN)
    else:
        view.copy_(values.float())
    return full, view


EXP_ULP = 2.0        # assumed: no accuracy table of expf ships with the ROCm documentation of this installation
DIV_ULP = 1.0        # hipcc divides fp32 correctly rounded by default (half an ulp); one is allowed


@pytest.mark.parametrize("rows,cols,pz,px", [(37, 39, 5, 2), (300, 128, 0, 0)], ids=["37x39-ldz44-ldx41", "300x128"])
def test_highway_kernels_match_float64_element_wise(dev, rows, cols, pz, px):
    """ops.highway_fwd / highway_bwd against float64, element by element, with first-order error propagation (u = 2^-24
    per rounding, 1 ulp = 2 u; expf is ASSUMED to be within 2 ulp: the installed ROCm documentation has no table):

      a = zt + bt           one rounding: |da| <= u |a|
      T = 1 / (1 + exp(-a)) |dT| <= T (1 - T) |da|  (sigma' = T (1 - T) <= 1/4)
                                    + T ((1 - T) 2 EXP_ULP u + u + 2 DIV_ULP u)      (expf, the sum, the division)
      H = max(zh + bh, 0)   |dH| <= u |zh + bh|
      y = H T + x (1 - T)   |dy| <= (|H| + |x|) |dT| + T |dH| + 2 u |H T| + 3 u |x| (1 - T)
    and for the backward pass, whose operands are the device's own T and H:
      dzt = dy (H - x) T (1 - T)   five roundings: gamma(5) |dzt|
      dzh = dy T where H > 0       one rounding; exactly 0 where H == 0
      dx (+)= dy (1 - T)           two roundings, three with the start value in the sum
    Second-order terms are covered by a factor 1 + 1e-4 (the largest relative error, of exp(-a) at |a| = 30, is 34 u)."""
    from neuralmonkey_amd import ops
    u = R.U
    g = torch.Generator().manual_seed(rows)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    bt, bh = (rnd(cols) * 0.5 - 1.0).float().double(), (rnd(cols) * 0.5).float().double()
    a = torch.rand(rows, cols, generator=g, dtype=torch.float64) * 60.0 - 30.0
    a[0, ::2], a[0, 1::2], a[1] = 30.0, -30.0, rnd(cols)                 # saturated gates, and ordinary ones
    zt = (a - bt).float().double()
    zh = rnd(rows, cols).float().double()
    zero = torch.zeros(rows, cols, dtype=torch.bool)
    zero.view(-1)[::7] = True
    zh = torch.where(zero, -bh.expand(rows, cols), zh)                   # zh + bh == 0 exactly
    x, dy = rnd(rows, cols).float().double(), rnd(rows, cols).float().double()
    a = zt + bt
    assert float(a.abs().max()) > 29.9 and float(a.abs().max()) < 30.01 and bool(((zh + bh) == 0)[zero].all())

    f32 = lambda t: t.float().contiguous().to(dev)
    zt_full, ztd = _padded2(rows, cols, pz, dev, zt)
    zh_full, zhd = _padded2(rows, cols, pz, dev, zh)
    x_full, xd = _padded2(rows, cols, px, dev, x)
    dy_full, dyd = _padded2(rows, cols, px, dev, dy)
    y_full, yd = _padded2(rows, cols, px, dev)
    tsave = torch.full((rows, cols), NAN, device=dev)
    hsave = torch.full((rows, cols), NAN, device=dev)
    ops.highway_fwd(ztd, zhd, xd, f32(bt), f32(bh), yd, tsave, hsave)
    torch.cuda.synchronize()

    t = torch.sigmoid(a)
    pre_h = zh + bh
    h = torch.relu(pre_h)
    so = 1.0 + 1e-4
    t_err = so * (t * (1 - t) * u * a.abs() + t * ((1 - t) * 2 * EXP_ULP * u + u + 2 * DIV_ULP * u)) + R.TINY
    h_err = so * u * pre_h.abs() + R.TINY
    y_err = so * ((h + x.abs()) * t_err + t * h_err + 2 * u * h * t + 3 * u * x.abs() * (1 - t)) + R.TINY
    label = "highway {}x{}".format(rows, cols)
    R.within_bound(tsave, t, t_err, label + " tsave", "highway tsave")
    R.within_bound(hsave, h, h_err, label + " hsave", "highway hsave")
    R.within_bound(yd, h * t + x * (1 - t), y_err, label + " y", "highway y")
    assert bool((hsave.cpu()[pre_h <= 0] == 0).all()) and bool((hsave.cpu()[pre_h > 0] > 0).all())

    td, hd = tsave.double().cpu(), hsave.double().cpu()                   # the backward pass's operands
    ref_dzt = dy * (hd - x) * td * (1 - td)
    ref_dzh = torch.where(hd > 0, dy * td, torch.zeros_like(dy))
    ref_d = dy * (1 - td)
    for accumulate in (False, True):
        dzt_full, dzt = _padded2(rows, cols, pz, dev)
        dzh_full, dzh = _padded2(rows, cols, pz, dev)
        start = 0.5 if accumulate else NAN
        dx_full, dx = _padded2(rows, cols, px, dev, torch.full((rows, cols), start))
        ops.highway_bwd(dyd, xd, tsave, hsave, dzt, dzh, dx, accumulate_dx=accumulate)
        torch.cuda.synchronize()
        tag = label + " acc {}".format(int(accumulate))
        R.within(dzt, ref_dzt, 5, ref_dzt.abs(), tag + " dzt", "highway dzt")
        R.within(dzh, ref_dzh, 1, ref_dzh.abs(), tag + " dzh", "highway dzh")
        assert bool((dzh.cpu()[hd == 0] == 0).all()) and bool((hd[zero] == 0).all())
        if accumulate:
            R.within(dx, ref_d + 0.5, 3, ref_d.abs() + 0.5, tag + " dx", "highway dx")
        else:
            R.within(dx, ref_d, 2, ref_d.abs(), tag + " dx", "highway dx")
        for full, pad_from in ((dzt_full, cols), (dzh_full, cols), (dx_full, cols)):
            assert bool((full[:, pad_from:] == 7.0).all())
    for full in (zt_full, zh_full, x_full, dy_full, y_full):
        assert bool((full[:, cols:] == 7.0).all())


def test_highway_kernels_take_no_rows(dev):
    from neuralmonkey_amd import ops
    cols = 39
    empty = lambda: torch.empty((0, cols), device=dev)
    bias = torch.zeros(cols, device=dev)
    ops.highway_fwd(empty(), empty(), empty(), bias, bias, empty(), empty(), empty())
    ops.highway_bwd(empty(), empty(), empty(), empty(), empty(), empty(), empty(), accumulate_dx=True)
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows,d", [(40, 39), (6400, 128), (130, 2100)])
def test_highway_layer_matches_float64(dev, rows, d):
    from neuralmonkey_amd import autodiff as F
    from neuralmonkey_amd import ops

    class _Ctx:                       # the tape needs buffers only
        device = dev
        session = type("Session", (), {})()

        def buffer(self, key, shape, dtype=torch.float32, zero=False):
            return torch.zeros(shape, dtype=dtype, device=dev)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(rows, d, generator=g, dtype=torch.float64)
    wt, wh = [torch.randn(d, d, generator=g, dtype=torch.float64) / math.sqrt(d) for _ in range(2)]
    bt, bh = [torch.randn(d, generator=g, dtype=torch.float64) * 0.5 - 1.0 for _ in range(2)]
    dy = torch.randn(rows, d, generator=g, dtype=torch.float64)
    tape = F.Tape(_Ctx(), "hw", recording=True)
    f32 = lambda t: t.float().contiguous().to(dev)
    v = lambda t: F.Var(f32(t), torch.zeros_like(f32(t)), True)
    xv = F.Var(f32(x), None, True)
    wtv, btv, whv, bhv = v(wt), v(bt), v(wh), v(bh)
    y = F.highway(tape, xv, wtv, btv, whv, bhv)
    y.grad = f32(dy)
    tape.backward()
    torch.cuda.synchronize()

    p = [t.clone().requires_grad_(True) for t in (x, wt, bt, wh, bh)]
    t_ = torch.sigmoid(p[0] @ p[1] + p[2])
    h_ = torch.relu(p[0] @ p[3] + p[4])
    ref = h_ * t_ + p[0] * (1 - t_)
    ref.backward(dy)
    scale = x.abs() @ wt.abs() + 1.0
    assert float(((y.data.double().cpu() - ref.detach()).abs() / scale).max()) < 1e-5
    for got, want in ((xv.grad, p[0].grad), (wtv.grad, p[1].grad), (btv.grad, p[2].grad), (whv.grad, p[3].grad),
                      (bhv.grad, p[4].grad)):
        err = (got.double().cpu() - want).abs().max() / (want.abs().max() + 1e-12)
        assert float(err) < 1e-5
    del ops


def _batches(dataset, n, size):
    from neuralmonkey_amd.dataset import BatchingScheme
    out = []
    for b in dataset.batches(BatchingScheme(batch_size=size)):
        out.append(b)
        if len(out) == n:
            break
    return out


def test_small_sent_cnn_ini_trains_decodes_and_round_trips(dev, cnn_root, tmp_path):  # noqa: F811
    from .test_reference_inis import load_verbatim
    model = load_verbatim(cnn_root, "small_sent_cnn", device=str(dev), seed=1234)
    tfm = model.tf_manager
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    step0 = tfm.sessions[0].global_step
    for batch in _batches(model.train_dataset, 3, model.batch_size):
        res = tfm.execute(batch, feedables, model.trainers, train=True)
        assert res[0].losses and all(np.isfinite(v) for v in res[0].losses.values()), res[0].losses
    assert tfm.sessions[0].global_step == step0 + 3
    val = _batches(model.val_dataset, 1, model.batch_size)[0]
    out = tfm.execute(val, feedables, model.runners, compute_losses=True)
    decoded = out[0].outputs["target"] if isinstance(out[0].outputs, dict) else out[0].outputs
    assert len(decoded) == len(val)
    for name in model.tf_manager.sessions[0].store.names():
        if name.startswith("sentence_encoder/"):
            assert bool(torch.isfinite(model.tf_manager.sessions[0].store[name]).all()), name
    path = str(tmp_path / "variables.data")
    tfm.save(path)
    again = load_verbatim(cnn_root, "small_sent_cnn", device=str(dev), seed=99)
    again.tf_manager.restore(path)
    out2 = again.tf_manager.execute(val, set.union(*[r.feedables for r in again.runners]), again.runners,
                                    compute_losses=False)
    decoded2 = out2[0].outputs["target"] if isinstance(out2[0].outputs, dict) else out2[0].outputs
    assert decoded2 == decoded


def test_a_sent_cnn_training_step_launches_no_torch_kernels(dev, cnn_root):  # noqa: F811
    from .test_no_foreign_kernels_gpu import _foreign_kernels
    from .test_reference_inis import load_verbatim
    model = load_verbatim(cnn_root, "small_sent_cnn", device=str(dev), seed=1234)
    tfm = model.tf_manager
    batch = _batches(model.train_dataset, 1, model.batch_size)[0]
    foreign = _foreign_kernels(lambda: tfm.execute(batch, model.trainers[0].feedables, model.trainers, train=True))
    assert not foreign, foreign
