"""nm_step_group (csrc/nm_step.hip) against float64 at the edges of every kernel instance behind it.

The cases, their inputs, the float64 reference and the bounds are in tests/step_group_cases.py.  For every case:

  * the kernel that runs is the one the case was written for -- asked of the library (ops.StepGroup.plan =
    nm_step_group_plan, the function nm_step_group itself launches by), so a tuning change that moves a case to another
    instance fails here instead of thinning the sweep;
  * every output matches float64 within the project's own bounds for these exact-fp32 MFMA sums (test_gemm,
    tests/test_kernels_gpu.py): 2e-6 sqrt(K) + 1e-6 of the largest reference magnitude for plain sums, 1e-5 behind a
    tanh, a gate or the blend;
  * writes stay inside [0, M) x [0, N): every output has 8 NaN rows below it and, where the descriptor has a leading
    dimension, 4 NaN columns beside it, which must still be NaN; the input half of an in-place state row is bit-unchanged;
  * row ids index 11-row tables, repeat, and are shared by rows of different workgroup tiles.

A planted permutation per a_kind-0 instance (one 1 per row of A, in columns spread over every K slice, and an asymmetric
Bt: C[i, j] must BE Bt[j, column of row i]) catches a swapped sub-tile, a swapped K slice or a wrong reduction slot that
a tolerance would average away.

NM_STEP_MEDIUM is read once per context, so test_switch_* runs the sweep in a fresh interpreter per value; inside it the
plan must obey the switch (0: no medium kernel; 2: 32x32 tiles only) and the results the same bounds."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import nm_oracle as O

from . import step_group_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEDIUM = ("medium-4x2x2", "medium-8x1x1", "medium-4x1x1")


def T(a, dev, dt=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)


def nans(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6))


@pytest.fixture(params=["register-staged", "lds-dma"])
def medium_path(request, monkeypatch):
    """NM_STEP_DMA 0 and 1 (read per call): under 1 a medium-M group whose every K is a multiple of 64 runs on
    step_group_dma_kernel, every other group on the kernel it runs on anyway."""
    monkeypatch.setenv("NM_STEP_DMA", "1" if request.param == "lds-dma" else "0")
    return request.param


def expected_plan(want, want_dma, medium_path, got):
    """The instance a case was written for under the default NM_STEP_MEDIUM; under the other two values (the child
    interpreters of test_switch_*) what the switch promises about the plan the library reports."""
    sw = os.environ.get("NM_STEP_MEDIUM", "1")
    if sw == "0":
        assert got in ("16x1", "16x2"), got
    elif sw == "2":
        assert got not in ("medium-4x2x2", "dma"), got
        assert (got in MEDIUM) == (want in MEDIUM)
    else:
        assert got == (want_dma if medium_path == "lds-dma" else want), got


def device_problem(m, p, x, dev):
    """(descriptor, {output name: (tensor, columns written)}, unchanged-input check) of one problem; outputs are NaN
    with PAD_ROWS rows below and, where there is a leading dimension, PAD_COLS columns beside the [m, n] that is written."""
    mp, pc = m + SC.PAD_ROWS, SC.PAD_COLS
    spec = dict(A=T(x["A"], dev), lda=x["A"].shape[1], Bt=T(x["Bt"], dev), ldb=x["Bt"].shape[1], N=p.n, K=p.k,
                epilogue=p.epilogue, act=p.act)
    outs, unchanged = {}, lambda: None
    if p.epilogue != SC.CAND:
        if p.bias:
            spec["bias"] = T(x["bias"], dev)
        if p.add:
            spec.update(add=T(x["add"], dev), ldadd=x["add"].shape[1])
            if p.ids:
                spec["add_ids"] = T(x["ids"], dev, torch.int32)
    if p.epilogue == SC.PLAIN:
        outs["C"] = (nans(dev, mp, p.n + pc), p.n)
        spec.update(C=outs["C"][0], ldc=p.n + pc)
    elif p.epilogue == SC.GATES:
        outs["ru"] = (nans(dev, mp, p.n), p.n)                       # (ru and rh have no leading dimension)
        outs["rh"] = (nans(dev, mp, p.n // 2), p.n // 2)
        spec.update(h=T(x["h"], dev), ldh=p.n // 2, ru=outs["ru"][0], rh=outs["rh"][0])
    else:
        # the state row of the decoder: [input half | state | pad]; in place, the new state replaces the old one
        ld = SC.IN_W + p.n + pc
        cat = nans(dev, mp, ld)
        cat[:m, :SC.IN_W] = T(x["input_half"], dev)
        cat[:m, SC.IN_W:SC.IN_W + p.n] = T(x["h"], dev)
        before = cat.clone()
        h = cat[:, SC.IN_W:]
        outs["h_out2"] = (nans(dev, mp, p.n + pc), p.n)
        spec.update(xc=T(x["xc"], dev), ldxc=x["xc"].shape[1], ru=T(x["ru_in"], dev), h=h, ldh=ld,
                    h_out2=outs["h_out2"][0], ldho2=p.n + pc)
        if p.ids:
            spec["xc_ids"] = T(x["ids"], dev, torch.int32)
        if p.inplace:
            outs["h_out"] = (h, p.n)                                 # (its pad columns and rows are NaN like any output's)
            spec.update(h_out=h, ldho=ld)
        else:
            outs["h_out"] = (nans(dev, mp, p.n + pc), p.n)
            spec.update(h_out=outs["h_out"][0], ldho=p.n + pc)

        def unchanged():
            now, was = cat.view(torch.int32), before.view(torch.int32)
            assert torch.equal(now[:, :SC.IN_W], was[:, :SC.IN_W])                      # the input half, bit for bit
            if not p.inplace:
                assert torch.equal(now, was)
    return spec, outs, unchanged


@pytest.mark.parametrize("case", SC.CASES, ids=[c.name for c in SC.CASES])
def test_sweep_case(dev, case, medium_path):
    from neuralmonkey_amd import ops
    data = SC.case_data(case)
    built = [device_problem(case.m, p, x, dev) for p, (x, _, _) in zip(case.probs, data)]
    group = ops.StepGroup(case.m, [spec for spec, _, _ in built])
    expected_plan(case.want, case.want_dma, medium_path, group.plan())
    group.launch()
    torch.cuda.synchronize()
    failures = []
    for i, (p, (_, ref, tol), (_, outs, unchanged)) in enumerate(zip(case.probs, data, built)):
        for name, (out, n) in outs.items():
            got = out.cpu().numpy()
            err = rel(got[:case.m, :n], ref[name])
            print("{}[{}] N={} K={} {}: error {:.3g}, bound {:.3g}".format(case.name, i, p.n, p.k, name, err, tol))
            if not err < tol:                                        # (a NaN inside the written block fails too)
                failures.append((i, name, err, tol))
            assert np.isnan(got[case.m:]).all(), (i, name, "rows beyond M were written")
            assert np.isnan(got[:, n:]).all(), (i, name, "columns beyond N were written")
        unchanged()
    assert not failures, failures


@pytest.mark.parametrize("name,m,n,k,want,dma", SC.PERMUTATIONS, ids=[c[0] for c in SC.PERMUTATIONS])
def test_planted_permutation_is_returned_exactly(dev, monkeypatch, name, m, n, k, want, dma):
    """K >= M, A[i, 37 i mod K] = 1 and nothing else: every sum has ONE non-zero term, so C[i, j] is Bt[j, 37 i mod K] to
    the bit, and the terms are spread over every K slice, every trip and every row and column sub-tile."""
    from neuralmonkey_amd import ops
    if os.environ.get("NM_STEP_MEDIUM", "1") != "1":
        want = None                                                  # (the children of test_switch_*: results only)
    monkeypatch.setenv("NM_STEP_DMA", "1" if dma else "0")
    a = np.zeros((m, k), np.float32)
    cols = (np.arange(m) * SC.PERM_STRIDE) % k
    assert k >= m and len(set(cols)) == m and cols.max() >= k - 16          # all distinct; the last 16-k chunk is used
    a[np.arange(m), cols] = 1.0
    bt = ((np.arange(n * k, dtype=np.int64).reshape(n, k) * 7 + 3) % 97).astype(np.float32) * 0.25
    assert not np.array_equal(bt[:m, cols], bt[:m, cols].T)
    out = nans(dev, m + SC.PAD_ROWS, n + SC.PAD_COLS)
    group = ops.StepGroup(m, [dict(A=T(a, dev), lda=k, Bt=T(bt, dev), ldb=k, N=n, K=k, epilogue=0, C=out,
                                   ldc=n + SC.PAD_COLS)])
    if want is not None:
        assert group.plan() == want
    group.launch()
    got = out.cpu().numpy()
    assert np.array_equal(got[:m, :n], bt[:, cols].T)
    assert np.isnan(got[m:]).all() and np.isnan(got[:, n:]).all()


def test_sweep_reaches_every_instance(dev, monkeypatch):
    """All seven instances are reached by the cases above -- by what the library says it would launch for the very
    descriptors the sweep launches (placeholders for the addresses), under the NM_STEP_DMA each case runs with."""
    from neuralmonkey_amd import ops
    seen = set()
    for dma in ("0", "1"):
        monkeypatch.setenv("NM_STEP_DMA", dma)
        for case in SC.CASES:
            plan = ops.StepGroup(case.m, SC.placeholder_specs(case)).plan()
            assert plan == (case.want_dma if dma == "1" else case.want), (case.name, dma)
            seen.add(plan)
    addr = 0x10000
    seen.add(ops.StepGroup(19, [dict(a_kind=1, Bt=addr, ldb=48, N=20, K=48, epilogue=0, act=1, C=addr, ldc=20, pctx=addr,
                                     pstat=addr, nchunk=6)]).plan())
    assert seen == set(ops.STEP_GROUP_PLANS)
    # a K that is no multiple of 64 under NM_STEP_DMA=1: the register-staged kernel (the last case of the DMA block)
    refused = [c for c in SC.CASES if c.name == "dma-refused-k-48"][0]
    assert refused.want_dma == refused.want and refused.want in MEDIUM


@pytest.mark.parametrize("bk,qpk,s,a,c,o", SC.PARTIALS)
def test_partials_of_six_and_eight_chunks(dev, bk, qpk, s, a, c, o):
    """a_kind 1 at 6 and 8 partials per row (the 8-wide instantiation of the loader), one and three queries per key
    batch: ctx . W + pre -> tanh and the attention distribution, (1) against float64 arithmetic on the very partials
    the launch read (SC.partials_reference: isolates the loader -- bound 1e-5 behind the tanh, as everywhere here) and
    (2) as test_partials_merged_in_the_operand_loader checks it, against the oracle's attention step end to end."""
    from neuralmonkey_amd import ops
    rng = np.random.default_rng([bk, qpk, s])
    r = bk * qpk
    q = rng.standard_normal((r, 40)).astype(np.float32)
    ap = {"query_w": (rng.standard_normal((40, a)) * 0.2).astype(np.float32),
          "query_b": (rng.standard_normal(a) * 0.1).astype(np.float32),
          "v": (rng.standard_normal(a) * 0.3).astype(np.float32), "bias": np.float32(0.1)}
    hf = rng.standard_normal((bk, s, a)).astype(np.float32)
    states = rng.standard_normal((bk, s, c)).astype(np.float32)
    mask = np.ones((bk, s), np.float32)
    for i in range(bk):
        mask[i, rng.integers(1, s + 1):] = 0
    mask[0] = 1                                                      # one sentence of full length: every partial counts
    rep = lambda x: np.repeat(x, qpk, axis=0)
    ctx_ref, w_ref = O.attention_step(q.astype(np.float64), rep(hf).astype(np.float64), rep(states).astype(np.float64),
                                      rep(mask).astype(np.float64), {k: np.asarray(v, np.float64) for k, v in ap.items()})
    wo = (rng.standard_normal((c, o)) / np.sqrt(c)).astype(np.float32)
    pre = rng.standard_normal((r, o)).astype(np.float32)
    nchunk, pctx_off, pstat_off = ops.attn_partials_layout(r, s, a, c)
    assert nchunk == -(-s // 12) and nchunk in (6, 8)
    ws = ops.attn_workspace(r, s, c, dev)
    y = T(q @ ap["query_w"] + ap["query_b"], dev)
    ops.attn_fwd_partials(y, T(hf, dev), T(states, dev), T(mask, dev), T(ap["v"], dev), T([ap["bias"]], dev), qpk, ws)
    out = nans(dev, r + SC.PAD_ROWS, o + SC.PAD_COLS)
    weights = nans(dev, r + SC.PAD_ROWS, s)
    group = ops.StepGroup(r, [dict(a_kind=1, Bt=T(wo.T, dev), ldb=c, N=o, K=c, epilogue=0, act=1, add=T(pre, dev),
                                   ldadd=o, C=out, ldc=o + SC.PAD_COLS, pctx=ws[pctx_off:], pstat=ws[pstat_off:],
                                   nchunk=nchunk, energies=ws, mask=T(mask, dev), weights=weights, S=s, mask_div=qpk,
                                   mask_mod=bk)])
    assert group.plan() == "16x1-partials"
    group.launch()
    host = ws.cpu().numpy()
    ctx64, w64 = SC.partials_reference(host[pctx_off:pctx_off + r * nchunk * c].reshape(r, nchunk, c),
                                       host[pstat_off:pstat_off + r * nchunk * 4].reshape(r, nchunk, 4),
                                       host[:r * s].reshape(r, s), rep(mask))
    got, got_w = out.cpu().numpy(), weights.cpu().numpy()
    err = rel(got[:r, :o], np.tanh(ctx64 @ wo.astype(np.float64) + pre))
    err_w = np.abs(got_w[:r] - w64).max()
    err_o = rel(got[:r, :o], np.tanh(ctx_ref @ wo.astype(np.float64) + pre))
    print("partials {} chunks, {} per key: loader {:.3g} (1e-5), weights {:.3g} (2e-6), end to end {:.3g} (1e-4)".format(
        nchunk, qpk, err, err_w, err_o))
    assert err < SC.TOL_ACT
    assert err_w < 2e-6 and np.abs(got_w[:r] - w_ref).max() < 2e-6
    assert err_o < 1e-4
    assert np.isnan(got[r:]).all() and np.isnan(got[:, o:]).all() and np.isnan(got_w[r:]).all()


def test_nine_partials_are_refused(dev):
    """Source length 97 makes nine partials: one more than the loader holds.  Plan and launch refuse alike, before any
    launch (the operands are never read)."""
    from neuralmonkey_amd import _lib, ops
    bk, qpk, s, a, c, o = SC.PARTIALS_REFUSED
    nchunk, pctx_off, pstat_off = ops.attn_partials_layout(bk * qpk, s, a, c)
    assert nchunk == 9
    ws = ops.attn_workspace(bk * qpk, s, c, dev)
    out = nans(dev, bk * qpk, o)
    group = ops.StepGroup(bk * qpk, [dict(a_kind=1, Bt=nans(dev, o, c), ldb=c, N=o, K=c, epilogue=0, act=1, C=out, ldc=o,
                                          pctx=ws[pctx_off:], pstat=ws[pstat_off:], nchunk=nchunk)])
    with pytest.raises(_lib.NMHipError, match="1..8 chunks"):
        group.plan()
    with pytest.raises(_lib.NMHipError, match="1..8 chunks"):
        group.launch()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


@pytest.mark.parametrize("switch", ["0", "2"])
def test_switch_medium(switch):
    """NM_STEP_MEDIUM=0 (16-row tiles at every M) and =2 (32x32 tiles only): the whole sweep and the planted
    permutations in a fresh interpreter (the switch is read once per context), where the plan must obey the switch."""
    env = dict(os.environ, NM_STEP_MEDIUM=switch)
    res = subprocess.run([sys.executable, "-m", "pytest", "tests/test_step_group_sweep_gpu.py", "-q", "-x", "-k",
                          "test_sweep_case or test_planted_permutation"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
