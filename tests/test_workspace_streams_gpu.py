"""Scratch that kernels re-use from call to call, on two streams at once.

ops._gemm_workspace (split-K slabs), ops._colsum_workspace (column-sum partials and arrival counters),
ops._layer_norm_bwd_workspace (the [G][2][D] partial sums between nm_layer_norm_bwd_params' two launches) and
ops.ctc_workspace (alphas between the loss and its gradient) are cached per (device, stream, workspace tag): launches of
one stream are ordered, launches of two streams -- side lanes, a second session, an ensemble, a captured graph replayed
beside the running batch (the tag) -- must not share a buffer.

The structural test is the deterministic one: two streams / two tags get buffers that do not overlap.  The behavioural
test launches each op on two streams in turn without synchronising and compares every result with float64 at the
tolerance of the op's single-stream test (tests/test_kernels_gpu.py: test_gemm, test_colsum_both_kernels,
test_layer_norm_bwd_with_parameter_gradients; tests/test_ctc_kernels_gpu.py); a race may pass it by luck, a correct
library never fails it."""
import numpy as np
import pytest
import torch

from . import test_ctc_kernels_gpu as C

pytestmark = pytest.mark.gpu

ROUNDS = 4


def _accessors(dev):
    from neuralmonkey_amd import ops
    return {"gemm": lambda: ops._gemm_workspace(dev),                          # pylint: disable=protected-access
            "colsum": lambda: ops._colsum_workspace(dev, 512),                 # pylint: disable=protected-access
            "layer_norm_bwd": lambda: ops._layer_norm_bwd_workspace(dev, 512),  # pylint: disable=protected-access
            "ctc": lambda: ops.ctc_workspace(7, 13, 6, dev)}


def _overlap(a, b):
    lo_a, lo_b = a.data_ptr(), b.data_ptr()
    return lo_a < lo_b + b.numel() * b.element_size() and lo_b < lo_a + a.numel() * a.element_size()


@pytest.mark.parametrize("which", ["gemm", "colsum", "layer_norm_bwd", "ctc"])
def test_streams_and_tags_get_workspaces_of_their_own(dev, which):
    from neuralmonkey_amd import ops
    get = _accessors(dev)[which]
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    assert s1.cuda_stream != s2.cuda_stream
    with torch.cuda.stream(s1):
        a, a_again = get(), get()
        old = ops.set_workspace_tag("second graph")
        try:
            a_tagged, a_tagged_again = get(), get()
        finally:
            ops.set_workspace_tag(old)
        a_after = get()
    with torch.cuda.stream(s2):
        b = get()
    torch.cuda.synchronize()
    for ws in (a, a_tagged, b):
        assert ws.numel() > 0
    assert a_again.data_ptr() == a.data_ptr() == a_after.data_ptr(), "same stream, same tag: the same buffer"
    assert a_tagged_again.data_ptr() == a_tagged.data_ptr()
    assert not _overlap(a, b), "two streams share a workspace"
    assert not _overlap(a, a_tagged), "two tags of one stream share a workspace"
    assert not _overlap(b, a_tagged)


def T(x, dev, dtype=torch.float32):
    return torch.tensor(np.asarray(x), dtype=dtype, device=dev)


def _two_streams(dev, launch):
    """``launch(stream index, round)`` on two streams in turn, ROUNDS times, nothing synchronised in between; both
    streams start after everything enqueued so far."""
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    torch.cuda.synchronize()
    for rnd in range(ROUNDS):
        for i, stream in enumerate(streams):
            with torch.cuda.stream(stream):
                launch(i, rnd)
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows,d", [(640, 2048), (37, 512)])
def test_layer_norm_backward_on_two_streams(dev, rows, d):
    from neuralmonkey_amd import ops
    cases = []
    for i in range(2):
        rng = np.random.default_rng(rows + d + 1000 * i)
        x = rng.standard_normal((rows, d)).astype(np.float32) * 2.0 + 0.5
        dy = rng.standard_normal((rows, d)).astype(np.float32) * (1.0 + 2.0 * i)
        gamma = (1.0 + 0.3 * rng.standard_normal(d)).astype(np.float32)
        beta = (0.1 * rng.standard_normal(d)).astype(np.float32)
        x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        g64 = torch.tensor(gamma, dtype=torch.float64, requires_grad=True)
        b64 = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
        mu = x64.mean(-1, keepdim=True)
        var = ((x64 - mu) ** 2).mean(-1, keepdim=True)
        y = (x64 - mu) * torch.rsqrt(var + 1e-6) * g64 + b64
        (y * torch.tensor(dy, dtype=torch.float64)).sum().backward()
        xd, dyd, gd, bd = T(x, dev), T(dy, dev), T(gamma, dev), T(beta, dev)
        out, mean, rstd = torch.empty_like(xd), torch.empty(rows, device=dev), torch.empty(rows, device=dev)
        ops.layer_norm_fwd(xd, gd, bd, out=out, mean=mean, rstd=rstd, eps=1e-6)
        outs = [(torch.full_like(xd, float("nan")), torch.zeros(d, device=dev), torch.zeros(d, device=dev))
                for _ in range(ROUNDS)]
        cases.append((xd, dyd, gd, mean, rstd, outs, (x64.grad.numpy(), g64.grad.numpy(), b64.grad.numpy())))

    def launch(i, rnd):
        xd, dyd, gd, mean, rstd, outs, _ = cases[i]
        dx, dgam, dbet = outs[rnd]
        ops.layer_norm_bwd_params(dyd, xd, mean, rstd, gd, dx, dgam, dbet, accumulate=False)
    _two_streams(dev, launch)
    tol = lambda ref: 2e-5 * max(1.0, float(np.abs(ref).max()))
    for i, case in enumerate(cases):
        want_dx, want_dg, want_db = case[6]
        for rnd, (dx, dgam, dbet) in enumerate(case[5]):
            assert np.abs(dx.cpu().numpy() - want_dx).max() <= tol(want_dx), (i, rnd)
            assert np.abs(dgam.cpu().numpy() - want_dg).max() <= tol(want_dg) * np.sqrt(rows), (i, rnd)
            assert np.abs(dbet.cpu().numpy() - want_db).max() <= tol(want_db) * np.sqrt(rows), (i, rnd)


@pytest.mark.parametrize("ta,tb", [(False, True), (True, False)])
def test_split_k_gemm_on_two_streams(dev, ta, tb):
    from neuralmonkey_amd import ops
    from .test_kernels_gpu import rel_err
    m, n, k, algo = 96, 136, 4096, 2                    # split-K on the 64 tile, ragged (tests/test_kernels_gpu.py)
    cases = []
    for i in range(2):
        rng = np.random.default_rng(m * 7 + n * 3 + k + i)
        a = rng.standard_normal((k, m) if ta else (m, k)).astype(np.float32)
        b = rng.standard_normal((n, k) if tb else (k, n)).astype(np.float32)
        ref = (a.T if ta else a).astype(np.float64) @ (b.T if tb else b).astype(np.float64)
        cases.append((T(a, dev), T(b, dev), ref, [torch.full((m, n), float("nan"), device=dev) for _ in range(ROUNDS)]))

    def launch(i, rnd):
        a, b, _, outs = cases[i]
        ops.gemm(a, b, out=outs[rnd], trans_a=ta, trans_b=tb, algo=algo)
    _two_streams(dev, launch)
    for i, (_, _, ref, outs) in enumerate(cases):
        for rnd, out in enumerate(outs):
            assert rel_err(out.cpu().numpy(), ref) < 2e-6 * np.sqrt(k) + 1e-6, (i, rnd)


@pytest.mark.parametrize("rows,cols", [(6400, 512), (63, 512)])        # the float4 kernel with row slices; the scalar one
def test_colsum_on_two_streams(dev, rows, cols):
    from neuralmonkey_amd import ops
    cases = []
    for i in range(2):
        rng = np.random.default_rng(rows + cols + i)
        full = (rng.standard_normal((rows, cols)) * (1.0 + i)).astype(np.float32)
        cases.append((T(full, dev), full.astype(np.float64).sum(0), 2e-6 * np.sqrt(rows) * max(1.0, np.abs(full).max()),
                      [torch.full((cols,), float("nan"), device=dev) for _ in range(ROUNDS)]))

    def launch(i, rnd):
        ops.colsum(cases[i][0], cases[i][3][rnd])
    _two_streams(dev, launch)
    for i, (_, want, tol, outs) in enumerate(cases):
        for rnd, out in enumerate(outs):
            assert np.abs(out.cpu().numpy() - want).max() <= tol, (i, rnd)
            assert torch.equal(out, outs[0]), "deterministic from launch to launch"


def test_ctc_loss_and_gradient_on_two_streams(dev):
    """The smallest shape of tests/test_ctc_kernels_gpu.py (T 13, B 7, K 3), one merge mode per stream: the gradient
    reads what the loss left in the stream's workspace."""
    from neuralmonkey_amd import ops
    names = ["k3_merge", "k3_plain"]
    cases = []
    for name in names:
        logits, labels, frame_lens, merge = C.make_case(name)
        lab, lab_len = C._device_labels(labels, dev)                    # pylint: disable=protected-access
        flen = torch.tensor(np.asarray(frame_lens, np.int32), device=dev)
        runs = [(torch.tensor(logits, device=dev), torch.full((logits.shape[1],), float("nan"), device=dev),
                 torch.full((1,), float("nan"), device=dev)) for _ in range(ROUNDS)]
        cases.append((lab, lab_len, flen, merge, runs, labels, frame_lens))

    def launch(i, rnd):
        lab, lab_len, flen, merge, runs, _, _ = cases[i]
        x, loss, total = runs[rnd]
        ws = ops.ctc_loss_fwd(x, lab, lab_len, flen, merge, loss, total)
        ops.ctc_loss_bwd(x, lab, lab_len, flen, x, ws, None)
    _two_streams(dev, launch)
    for name, (_, _, _, merge, runs, labels, frame_lens) in zip(names, cases):
        exp = C.expectations(name)
        for x, loss, total in runs:
            C._check(name, exp, loss.cpu().numpy().astype(np.float64), float(total.cpu()[0]),          # pylint: disable=protected-access
                     x.cpu().numpy().astype(np.float64), labels, frame_lens, merge)
