"""nm_conv2d_act_fwd (csrc/nm_vgg.hip) against a float64 convolution that torch computes on the CPU
(tests/imagenet_ref.py).  Inputs, filters and biases have both signs, so the ReLU cuts about half of the outputs.

Bound, per element: |got - want| <= K * 2^-24 * (sum |x||w| + |b|) with K = k*k*Cin + 1 -- the forward error of a
length-K fp32 sum of exactly rounded products in ANY order (gamma_K = K u / (1 - K u) with u = 2^-24; K u < 3e-4 here,
and the products enter fused, so the plain K u holds with room); the ReLU does not widen it (|max(a, 0) - max(b, 0)| <=
|a - b|).  sum |x||w| comes from the same reference run on the absolute values.

The shapes are the smallest at which the flattened tiling can go wrong (tiles are 128 or 64 positions by 64 channels,
chunks hold 16 values of the flattened (ky, kx, ci)):
  a  3 x 5x7,   k 3 SAME, 3 -> 8     105 positions: tiles span rows and images; K = 27, the scalar gather; Cout < a tile
  b  2 x 14x14, k 3 SAME, 16 -> 72   Cout tail past 64; ReLU on and off
  c  1 x 1x1,   k 3 SAME, 8 -> 8     all halo
  d  2 x 9x130, k 3 SAME, 20 -> 32   a row longer than a tile; Cin no multiple of the chunk: a chunk spans two taps
  e  2 x 3x3,   k 1,      24 -> 40   the 1 x 1 form
  f  2 x 7x7 and 9x8, k 7 VALID, 8 -> 16   outputs 1x1 and 3x2
  g  as b with ldx > Cin, ldy > Cout and no bias, with paddings that keep and that break the 16-byte loads
  h  1 x 14x14, k 3 SAME, 512 -> 512 the real conv5 width, once
Every case runs under each of the two tiles and under the automatic choice."""
import numpy as np
import pytest
import torch

from . import imagenet_ref as ref

pytestmark = pytest.mark.gpu

TILES = [None, "128x64", "64x64"]
CASES = {
    "a": (3, 5, 7, 3, "same", 3, 8),
    "b": (2, 14, 14, 3, "same", 16, 72),
    "c": (1, 1, 1, 3, "same", 8, 8),
    "d": (2, 9, 130, 3, "same", 20, 32),
    "e": (2, 3, 3, 1, "valid", 24, 40),
    "f1": (2, 7, 7, 7, "valid", 8, 16),
    "f2": (2, 9, 8, 7, "valid", 8, 16),
    "h": (1, 14, 14, 3, "same", 512, 512),
}
_MEMO = {}


def problem(case):
    """(x, filt, bias, want with bias (no ReLU), magnitude sum |x||w|), computed once per case."""
    if case not in _MEMO:
        bsz, h, w, k, padding, cin, cout = CASES[case]
        rng = np.random.default_rng(sum(map(ord, case)) + 17)
        x = rng.uniform(-1.0, 1.0, (bsz, h, w, cin)).astype(np.float32)
        filt = rng.uniform(-1.0, 1.0, (k, k, cin, cout)).astype(np.float32)
        bias = rng.uniform(-1.0, 1.0, (cout,)).astype(np.float32)
        linear = ref.conv2d(x, filt, None, padding, False)
        mag = ref.conv2d(np.abs(x), np.abs(filt), None, padding, False)
        for arr in (x, filt, bias, linear, mag):
            arr.setflags(write=False)
        _MEMO[case] = (x, filt, bias, linear, mag)
    return _MEMO[case]


def check(case, got, want, mag, bias_mag, label):
    _, _, _, k, _, cin, _ = CASES[case]
    bound = (k * k * cin + 1) * 2.0 ** -24 * (mag + bias_mag)
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("conv2d_act {} {}: max |err| {:.3e}, worst err / bound {:.3f}".format(case, label, float(err.max()), worst))
    assert got.shape == want.shape and np.isfinite(got).all()
    assert (err <= bound).all(), (case, label, worst)


@pytest.mark.parametrize("case", sorted(CASES))
def test_conv2d_act_meets_the_fp32_sum_bound(dev, case):
    from neuralmonkey_amd import ops
    bsz, h, w, k, padding, cin, cout = CASES[case]
    x, filt, bias, linear, mag = problem(case)
    oh, ow = ops.conv2d_out_hw(h, w, k, padding)
    assert linear.shape == (bsz, oh, ow, cout)
    if case == "f1":
        assert (oh, ow) == (1, 1)
    if case == "f2":
        assert (oh, ow) == (3, 2)
    xd, fd, bd = (torch.from_numpy(np.array(v)).to(dev) for v in (x, filt, bias))
    with_bias = linear + bias.astype(np.float64)
    want = np.maximum(with_bias, 0.0)
    assert 0.2 < (with_bias < 0).mean() < 0.8                      # the ReLU matters
    for tile in TILES if case != "h" else [None, "128x64"]:
        y = torch.full((bsz, oh, ow, cout), float("nan"), device=dev)
        ops.conv2d_act_fwd(xd, fd, bd, y, padding, relu=True, tile=tile)
        check(case, y.cpu().numpy(), want, mag, np.abs(bias.astype(np.float64)), "relu tile {}".format(tile))
    if case == "b":                                                # ... and with the ReLU off
        y = torch.full((bsz, oh, ow, cout), float("nan"), device=dev)
        ops.conv2d_act_fwd(xd, fd, bd, y, padding, relu=False)
        got = y.cpu().numpy()
        check(case, got, with_bias, mag, np.abs(bias.astype(np.float64)), "linear")
        assert (got < 0).any()


@pytest.mark.parametrize("pad_x, pad_y", [(4, 8), (3, 5)])
def test_leading_dimensions_and_a_null_bias(dev, pad_x, pad_y):
    """Case g: (b) read from and written into wider buffers, without a bias; what lies beyond Cout is not touched.  A
    padding of 4 keeps the rows 16-byte aligned (the vector gather), one of 3 does not (the scalar gather)."""
    from neuralmonkey_amd import ops
    bsz, h, w, k, padding, cin, cout = CASES["b"]
    x, filt, _, linear, mag = problem("b")
    xw = torch.full((bsz, h, w, cin + pad_x), 7.0, device=dev)
    xw[..., :cin] = torch.from_numpy(np.array(x)).to(dev)
    yw = torch.full((bsz, h, w, cout + pad_y), -3.0, device=dev)
    fd = torch.from_numpy(np.array(filt)).to(dev)
    for tile in TILES:
        yw.fill_(-3.0)
        ops.conv2d_act_fwd(xw[..., :cin], fd, None, yw[..., :cout], padding, relu=True, tile=tile)
        got = yw.cpu().numpy()
        assert (got[..., cout:] == -3.0).all()
        check("b", got[..., :cout], np.maximum(linear, 0.0), mag, 0.0, "ld +{} +{} tile {}".format(pad_x, pad_y, tile))


def test_two_runs_are_bit_equal(dev):
    from neuralmonkey_amd import ops
    bsz, h, w, k, padding, cin, cout = CASES["b"]
    x, filt, bias, _, _ = problem("b")
    xd, fd, bd = (torch.from_numpy(np.array(v)).to(dev) for v in (x, filt, bias))
    runs = []
    for _ in range(2):
        y = torch.zeros((bsz, h, w, cout), device=dev)
        ops.conv2d_act_fwd(xd, fd, bd, y, padding, relu=True)
        runs.append(y.cpu().numpy().tobytes())
    assert runs[0] == runs[1]
