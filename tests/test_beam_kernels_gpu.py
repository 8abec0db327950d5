"""The three beam step kernels of csrc/nm_logits.hip -- nm_beam_topk_step (two passes; also in the ensemble convention:
log-probabilities with zero row statistics), nm_beam_topk_step_fused (register-resident row scan, with its two-pass
fallback for k > 8, V % 4 != 0, unaligned rows and V > 131072) and nm_beam_topk_step_tiles (tile statistics, both tile
widths) -- each against the float64 restatement of the beam body (oracle/beam_ref.py), on the case table of
tests/beam_cases.py.  No kernel is compared with another kernel here.

Acceptance (oracle/beam_ref.py:check_step, every sentence, none excused), with tol(c) = C * (1 + |S_c|) over the
float64 scores S and S_k the k-th largest: the k flat indices are in range and distinct; out_score within tol of S at
the returned index, non-increasing, equal neighbours in ascending flat index; every candidate with
S_c - tol(c) > S_k + tol(k) is returned and every returned one has S_c + tol(c) >= S_k - tol(k); lengths, finished and
src_row are exactly the state derived from the returned indices, logprob_sum within C * (1 + |hyp|); rmax_out equals
the float32 row maximum and rlse_out lies within C * (1 + |lse|) in live rows; all_finished preset to 1 ends as
int(all out_finished), preset to 0 stays 0.  The structural-tie cases add the exact expected selection (float64 scores,
lower flat index wins exact equality, first-step rows by the rounded-sum rule).

C = 3.52e-6: 16 x 2.2e-7, which bounds the worst |float32 restatement - float64| / (1 + |score|) measured over the
table on the CPU, 2.13e-7, the runs with the lse moved by +-2 ulp included (tests/test_beam_ref.py); the cap of 1e-5
does not bind.  In every general case the band at the boundary holds the k-th candidate alone (asserted there), so the
rule pins the selected set.

Before every call the workspace is filled with 0xFF bytes and every output with a sentinel, and every row is followed
by ``pad`` columns of +3e38: an unwritten slot, an unwritten output or a read past the end of a row shows.  Where a
kernel leaves one candidate list per row (tiles; fused outside its fallback), the workspace behind the lists must
still hold the 0xFF bytes: a write past a row's list lands in the next row's and is otherwise seen only when that row
loses a race.

Mutations of csrc/nm_logits.hip that these tests were checked to catch are listed in DESIGN.md next to the kernels."""
import numpy as np
import pytest
import torch

from oracle import beam_ref as R

from . import beam_cases as BC

pytestmark = pytest.mark.gpu
OUTS = ("score", "word", "beam", "logprob_sum", "lengths", "finished", "src_row")
BIG = 3e38


def _t(a, dev, dt=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)


def _padded(dev, x, pad):
    """The rows of ``x`` inside a buffer whose row stride is V + pad; the padding columns hold +3e38."""
    rows, v = x.shape
    buf = torch.full((rows, v + pad), BIG, device=dev)
    view = buf[:, :v]
    view.copy_(_t(x, dev))
    assert view.stride(0) == v + pad
    return view


def _launch(dev, o, kern, ld, stats, preset):
    """One call of the kernel under test on fresh sentinels; returns the outputs as NumPy arrays."""
    from neuralmonkey_amd import ops
    c = o.case
    b, k, v, rows = c.b, c.k, c.v, c.b * c.k
    lps, lens = _t(o.lps, dev), _t(o.lens, dev, torch.int32)
    fin, pen = _t(o.fin.astype(np.int32), dev, torch.int32), _t(o.penalty, dev)
    out = [torch.full((b, k), float("nan"), device=dev) if n in ("score", "logprob_sum") else
           torch.full((b, k), -77, dtype=torch.int32, device=dev) for n in OUTS]
    ws = ops.beam_workspace(b, k, v, dev)
    ws.view(torch.int32).fill_(-1)                                   # 0xFF bytes
    mx, lse = torch.full((rows,), float("nan"), device=dev), torch.full((rows,), float("nan"), device=dev)
    af = torch.full((1,), preset, dtype=torch.int32, device=dev)
    if kern == "twopass":
        ops.row_stats(ld, mx, lse, None)
        ops.beam_topk_step(ld, b, k, mx, lse, lps, lens, fin, pen, c.end, *out, ws, all_finished=af)
    elif kern == "ensemble":
        mx, lse = _t(o.rmax, dev), _t(o.rlse, dev)
        ops.beam_topk_step(ld, b, k, mx, lse, lps, lens, fin, pen, c.end, *out, ws, all_finished=af)
    elif kern == "fused":
        ops.beam_topk_step_fused(ld, b, k, lps, lens, fin, pen, c.end, *out, ws, mx, lse, all_finished=af)
    else:
        tile = {"tiles64": 64, "tiles128": 128, "tiles_gemm": None}[kern]
        ops.beam_topk_step_tiles(ld, stats, b, k, lps, lens, fin, pen, c.end, *out, ws, mx, lse, all_finished=af,
                                 tile=tile)
    got = {n: t.cpu().numpy() for n, t in zip(OUTS, out)}
    got["all_finished"] = int(af.item())
    if kern != "fused" or (k <= 8 and v % 4 == 0 and c.pad % 4 == 0 and v <= 131072):
        if kern not in ("twopass", "ensemble"):
            # one list of K = 4 / 8 / 16 entries per row (scores, then indices at B * 64 * 16): nothing behind them
            lists, half = rows * (4 if k <= 4 else 8 if k <= 8 else 16), b * 64 * 16
            w = ws.view(torch.int32).cpu().numpy()
            got["stray"] = int((w[lists:half] != -1).sum() + (w[half + lists:2 * half] != -1).sum())
    if kern != "ensemble":
        got["rmax"], got["rlse"] = mx.cpu().numpy(), lse.cpu().numpy()
    return got


def _check(o, kern, got, again):
    """``got``: the call with all_finished preset to 1; ``again``: the same call with the word preset to 0."""
    got["all_finished_from0"] = again["all_finished"]
    assert got.pop("stray", 0) == 0, "{} / {}: workspace written behind the row lists".format(o.case.name, kern)
    problems = R.check_step(o.ref, got, BC.C, o.exact)
    assert problems == [], "{} / {}: {}".format(o.case.name, kern, problems)


@pytest.mark.parametrize("name,kern", BC.RUNS, ids=["{}-{}".format(n, kn) for n, kn in BC.RUNS])
def test_step_against_float64(dev, name, kern):
    o = BC.build(name)
    c = o.case
    ld = _padded(dev, o.logits, c.pad)
    stats = None
    if kern.startswith("tiles"):
        st = R.tile_stats(o.logits, int(kern[5:]))
        stats = _t(st.view(np.int32), dev, torch.int32).view(torch.float32)     # (bit copy: the argmax is an int)
    _check(o, kern, _launch(dev, o, kern, ld, stats, 1), _launch(dev, o, kern, ld, stats, 0))


def test_tiles_through_the_stats_gemm_at_the_width_the_library_picks(dev):
    """More than 256 rows: nm_logits_stats_tile gives 128.  The logits are planted through an identity product, the
    GEMM's own records are what tile_stats builds (max and argmax exactly, sums to 1e-6), and the step is held to the
    float64 rule."""
    from neuralmonkey_amd import _lib, ops
    o = BC.build(BC.GEMM_CASE.name)
    c = o.case
    rows, v = o.logits.shape
    assert rows > 256 and int(_lib.load().nm_logits_stats_tile(rows)) == 128
    kpad = (rows + 3) // 4 * 4
    eye = np.zeros((rows, kpad), np.float32)
    eye[np.arange(rows), np.arange(rows)] = 1.0
    lpad = np.zeros((kpad, v), np.float32)
    lpad[:rows] = o.logits
    stats = ops.logits_stats_buffer(rows, v, dev)
    stats.view(torch.int32).fill_(-1)
    ld = torch.full((rows, v), float("nan"), device=dev)
    ops.logits_stats_gemm(_t(eye, dev), _t(lpad, dev), None, stats, out=ld)
    assert np.array_equal(ld.cpu().numpy(), o.logits)
    want = R.tile_stats(o.logits, 128)
    nt = want.shape[1]
    got = stats.view(torch.int32).cpu().numpy()[:rows * nt * 4].view(np.float32).reshape(rows, nt, 4)
    assert np.array_equal(got[:, :, 0], want[:, :, 0])
    assert np.array_equal(got[:, :, 2].copy().view(np.int32), want[:, :, 2].copy().view(np.int32))
    assert (np.abs(got[:, :, 1] - want[:, :, 1]) <= 1e-6 * np.maximum(1.0, want[:, :, 1])).all()
    _check(o, "tiles_gemm", _launch(dev, o, "tiles_gemm", ld, stats, 1), _launch(dev, o, "tiles_gemm", ld, stats, 0))
