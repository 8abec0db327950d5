"""The LDS-ring loop of the 128x128 fp32 GEMM (gemm_ring, neuralmonkey_amd/csrc/nm_gemm.hip) against the loop it
replaces (gemm_tiled<4, 2, 1, 2, ..., 16>): the same k-ascending MFMA chain per output element, the same split-K
slices, slabs and epilogue, so the two must agree BIT FOR BIT on the whole output buffer (columns beyond N, where
ldc > N, stay the NaN they were filled with).  The same outputs are held against float64 at test_gemm's tolerances.

Both loops run in one process: the calls go through a library context created under NM_GEMM_CFG=10 (the ring,
whatever the default is), ``algo=1`` takes that context's loop and ``algo=5`` forces gemm_tiled's.

Shapes are the smallest at which a three-stage ring can go wrong: 1, 2, 3, 4, 5 and 7 k-tiles (prologue, drain, wrap),
K tails, the scalar-load path (odd leading dimensions), ragged and multi-tile (M, N), every layout, every epilogue,
a strided batch, and split-K through the default workspace.  Split factors of the makespan model (nm_gemm_f32) with
128x128 tiles and the default 128 MB workspace, k-tiles per slice in brackets:
    (128, 128, 2064)  129 k-tiles  15 slices [9 x 14, 3]
    (128, 256, 1040)   65 k-tiles   8 slices [9 x 7, 2]
    (640, 512, 8192)  512 k-tiles  12 slices [43 x 11, 39]
The model never leaves a slice empty; 16 slices of (128, 128, 2064) do ([9 x 14, 3, 0]: slice 15 starts beyond K and
must store a slab of zeros without loading anything), so that case runs under a context with NM_GEMM_SK=16 too, and
(128, 128, 1168) adds a last slice of ONE k-tile (9 slices, [9 x 8, 1])."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RING, OLD = 1, 5                 # nm_gemm_f32 algo: 128x128 tiles with the context's loop / with gemm_tiled's loop
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]
SHAPES_MN = [(128, 128), (130, 132), (1, 5), (257, 129)]


@contextlib.contextmanager
def ring_context(**switches):
    """Library calls of this thread inside the block run under a context that read NM_GEMM_CFG=10 (+ ``switches``)."""
    from neuralmonkey_amd import _lib
    lib = _lib.load()
    switches = dict(switches, NM_GEMM_CFG=10)
    default = lib.nm_ctx_current()
    saved = {name: os.environ.get(name) for name in switches}
    ctx = ctypes.c_void_p()
    try:
        for name, value in switches.items():
            os.environ[name] = str(value)
        assert lib.nm_create(-1, ctypes.byref(ctx)) == 0 and ctx.value, lib.nm_last_error()
        for name, value in switches.items():
            got = ctypes.c_int(-12345)
            assert lib.nm_ctx_switch(ctx, name[3:].lower().encode(), ctypes.byref(got)) == 0, lib.nm_last_error()
            assert got.value == value, (name, value, got.value)
        assert lib.nm_ctx_bind(ctx) == 0, lib.nm_last_error()
        yield
    finally:
        lib.nm_ctx_bind(None)
        if ctx.value:
            lib.nm_destroy(ctx)
        for name, old in saved.items():
            if old is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = old
        assert lib.nm_ctx_current() == default


@pytest.fixture
def ring(dev):
    with ring_context():
        yield dev


def rel_err(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-6))


def operand(rng, rows, cols, dev, odd_ld=False, batch=None):
    """A [rows, cols] operand (or [batch, rows, cols]) as a view into a wider buffer: leading dimension cols + 4, or
    the next odd number when ``odd_ld`` (rows then start at unaligned addresses: the scalar-load path)."""
    ld = cols + 4 + (cols % 2 == 0) if odd_ld else (cols + 3) // 4 * 4 + 4
    lead = () if batch is None else (batch,)
    host = rng.standard_normal(lead + (rows, cols)).astype(np.float32)
    buf = torch.zeros(lead + (rows, ld), device=dev)
    buf[..., :cols] = torch.from_numpy(host).to(dev)
    return host, buf[..., :cols]


def both_loops(dev, a, b, ta, tb, m, n, ldc, bias=None, act=None, c0=None, batch=None):
    """The product through the ring and through gemm_tiled's loop: (ring's [.., m, n] block on the host, after the whole
    buffers, NaN padding included, compared equal as bit patterns)."""
    from neuralmonkey_amd import ops
    outs = []
    for algo in (RING, OLD):
        lead = () if batch is None else (batch,)
        buf = torch.full(lead + (m, ldc), float("nan"), device=dev)
        if c0 is not None:
            buf[..., :n] = c0
        ops.gemm(a, b, out=buf[..., :n], bias=bias, act=act, trans_a=ta, trans_b=tb, accumulate=c0 is not None,
                 algo=algo)
        outs.append(buf)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "ring and gemm_tiled differ"
    if ldc > n:
        assert bool(torch.isnan(outs[0][..., n:]).all()), "written beyond N"
    return outs[0][..., :n].cpu().numpy()


def check_case(dev, rng, m, n, k, ta, tb, epilogues, odd_ld=False, ldc=None, batch=None):
    ldc = n + 3 if ldc is None else ldc
    a, a_dev = operand(rng, *((k, m) if ta else (m, k)), dev, odd_ld, batch)
    b, b_dev = operand(rng, *((n, k) if tb else (k, n)), dev, odd_ld, batch)
    swap = lambda x: np.swapaxes(x, -1, -2)
    a64, b64 = (swap(a) if ta else a).astype(np.float64), (swap(b) if tb else b).astype(np.float64)
    ref = a64 @ b64
    what = "m={} n={} k={} ta={} tb={} odd_ld={} batch={}".format(m, n, k, ta, tb, odd_ld, batch)
    tol = 2e-6 * np.sqrt(k) + 1e-6                                   # test_gemm's
    out = both_loops(dev, a_dev, b_dev, ta, tb, m, n, ldc, batch=batch)
    assert rel_err(out, ref) < tol, what
    if not epilogues:
        return
    bias = rng.standard_normal(n).astype(np.float32)
    bias_dev = torch.from_numpy(bias).to(dev)
    c0 = rng.standard_normal(ref.shape).astype(np.float32)
    out = both_loops(dev, a_dev, b_dev, ta, tb, m, n, ldc, c0=torch.from_numpy(c0).to(dev), batch=batch)
    assert rel_err(out, ref + c0) < tol, what + " accumulate"
    a_s = (a / np.sqrt(k)).astype(np.float32)                        # O(1) pre-activations
    a_dev.copy_(torch.from_numpy(a_s))
    ref_s = (swap(a_s) if ta else a_s).astype(np.float64) @ b64
    out = both_loops(dev, a_dev, b_dev, ta, tb, m, n, ldc, bias=bias_dev, act="tanh", batch=batch)
    assert rel_err(out, np.tanh(ref_s + bias)) < 1e-5, what + " bias + tanh"
    out = both_loops(dev, a_dev, b_dev, ta, tb, m, n, ldc, bias=bias_dev, act="relu", batch=batch)
    assert rel_err(out, np.maximum(ref_s + bias, 0.0)) < 1e-5, what + " bias + relu"


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_k_tiles_and_tails(ring, ta, tb):
    """1, 2, 3, 4, 5, 7 k-tiles and the K tails 4, 20, 36, 52 at every (M, N); the epilogues at three tiles and at
    three tiles + a tail."""
    rng = np.random.default_rng(100 + 2 * ta + tb)
    for k in (16, 32, 48, 64, 80, 112, 4, 20, 36, 52):
        for m, n in SHAPES_MN:
            check_case(ring, rng, m, n, k, ta, tb, epilogues=k in (48, 52))


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_scalar_load_path(ring, ta, tb):
    """Odd leading dimensions (and K, M, N that are no multiples of 4): every element loaded on its own."""
    rng = np.random.default_rng(200 + 2 * ta + tb)
    for k in (1, 17, 50):
        for m, n in SHAPES_MN:
            check_case(ring, rng, m, n, k, ta, tb, epilogues=k == 50, odd_ld=True)


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_batch_of_three_with_strides(ring, ta, tb):
    rng = np.random.default_rng(300 + 2 * ta + tb)
    check_case(ring, rng, 130, 132, 52, ta, tb, epilogues=True, batch=3)
    check_case(ring, rng, 257, 129, 80, ta, tb, epilogues=False, batch=3)


@pytest.mark.parametrize("ta,tb", [(False, False), (True, False)])
@pytest.mark.parametrize("m,n,k", [(128, 128, 2064), (128, 256, 1040), (640, 512, 8192), (128, 128, 1168)])
def test_split_k_through_the_default_workspace(ring, m, n, k, ta, tb):
    rng = np.random.default_rng(m + n + k + 2 * ta + tb)
    check_case(ring, rng, m, n, k, ta, tb, epilogues=True)


@pytest.mark.parametrize("ta,tb", [(False, False), (True, False)])
def test_split_k_with_an_empty_last_slice(dev, ta, tb):
    """(128, 128, 2064) over 16 slices of 9 k-tiles: slice 14 has three, slice 15 none."""
    rng = np.random.default_rng(400 + 2 * ta + tb)
    with ring_context(NM_GEMM_SK=16):
        check_case(dev, rng, 128, 128, 2064, ta, tb, epilogues=True)
        check_case(dev, rng, 130, 132, 2064, ta, tb, epilogues=False)
