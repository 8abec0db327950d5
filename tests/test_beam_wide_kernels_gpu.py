"""nm_beam_topk_step_wide (csrc/nm_logits.hip) against the float64 restatement of the beam body
(oracle/beam_ref.py) on the case table of tests/beam_wide_cases.py, in every convention a case names: statistics
computed by the kernel, given from ops.row_stats, the ensemble convention (log-probabilities, zero statistics), and
tile statistics 64 and 128 columns wide.  No kernel is compared with another kernel.

The protocol is that of tests/test_beam_kernels_gpu.py: outputs preset to sentinels, the workspace filled with 0xFF
bytes, ``pad`` columns of +3e38 behind every row, the call made twice (all_finished preset to 1 and to 0), acceptance
by oracle/beam_ref.py:check_step with C = 3.52e-6 in every sentence, none excused, the exact expected selection in the
structural-tie cases; rmax_out equal to the float32 row maximum and rlse_out within C * (1 + |lse|) in live rows
wherever the kernel writes them.  tests/test_beam_wide_ref.py shows on the CPU that the float32 restatement meets the
rule on this table and that the band at the boundary holds the k-th candidate alone in every sentence of every
general case, at its own k and at k = 16.

The tie cases and the first-step sentences overflow the candidate buffer and go through the kernel's exact streaming
path; the other sentences go through the counting passes."""
import numpy as np
import pytest
import torch

from oracle import beam_ref as R

from . import beam_wide_cases as WC

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


def _inputs(dev, o):
    return (_t(o.lps, dev), _t(o.lens, dev, torch.int32), _t(o.fin.astype(np.int32), dev, torch.int32),
            _t(o.penalty, dev))


def _sentinels(dev, b, k):
    return [torch.full((b, k), float("nan"), device=dev) if n in ("score", "logprob_sum") else
            torch.full((b, k), -77, dtype=torch.int32, device=dev) for n in OUTS]


def _launch(dev, o, kern, ld, preset):
    """One call of the wide entry on fresh sentinels; returns the outputs as NumPy arrays."""
    from neuralmonkey_amd import ops
    c = o.case
    b, k, v, rows = c.b, c.k, c.v, c.b * c.k
    lps, lens, fin, pen = _inputs(dev, o)
    out = _sentinels(dev, b, k)
    ws = ops.beam_workspace(b, k, v, dev)
    ws.view(torch.int32).fill_(-1)                                   # 0xFF bytes
    mx, lse = torch.full((rows,), float("nan"), device=dev), torch.full((rows,), float("nan"), device=dev)
    af = torch.full((1,), preset, dtype=torch.int32, device=dev)
    kw = {}
    if kern == "given":
        gm, gl = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
        ops.row_stats(ld, gm, gl, None)
        kw = {"rmax_in": gm, "rlse_in": gl}
    elif kern == "ensemble":
        kw = {"rmax_in": _t(o.rmax, dev), "rlse_in": _t(o.rlse, dev)}
    elif kern.startswith("tiles"):
        st = R.tile_stats(o.logits, int(kern[5:]))
        kw = {"stats": _t(st.view(np.int32), dev, torch.int32).view(torch.float32), "tile": int(kern[5:])}
    ops.beam_topk_step_wide(ld, b, k, lps, lens, fin, pen, c.end, *out, ws, mx, lse, all_finished=af, **kw)
    got = {n: t.cpu().numpy() for n, t in zip(OUTS, out)}
    got["all_finished"] = int(af.item())
    if kern in ("computed", "tiles64", "tiles128"):
        got["rmax"], got["rlse"] = mx.cpu().numpy(), lse.cpu().numpy()
    return got


@pytest.mark.parametrize("name,kern", WC.RUNS, ids=["{}-{}".format(n, kn) for n, kn in WC.RUNS])
def test_wide_step_against_float64(dev, name, kern):
    o = WC.build(name)
    ld = _padded(dev, o.logits, o.case.pad)
    got, again = _launch(dev, o, kern, ld, 1), _launch(dev, o, kern, ld, 0)
    got["all_finished_from0"] = again["all_finished"]
    problems = R.check_step(o.ref, got, WC.C, o.exact)
    assert problems == [], "{} / {}: {}".format(name, kern, problems)
    # determinism: the two calls (different all_finished presets, fresh workspaces) agree bit for bit
    for n in OUTS + (("rmax", "rlse") if "rmax" in got else ()):
        assert np.array_equal(got[n].view(np.int32), again[n].view(np.int32)), (name, kern, n)


def _small(dev):
    o = WC.build("w_k17_v70")
    return o, _padded(dev, o.logits, 0), _inputs(dev, o)


@pytest.mark.parametrize("what", ["k0", "k65", "kv_2_31", "short_workspace", "null_output", "ldx_below_v"])
def test_refusals_return_an_error_and_launch_nothing(dev, what):
    from neuralmonkey_amd import _lib, ops
    o, ld, (lps, lens, fin, pen) = _small(dev)
    c = o.case
    b, k, v = c.b, c.k, c.v
    out = _sentinels(dev, b, 65)
    lib = _lib.load()
    need = int(lib.nm_beam_workspace_bytes(b, k, v))
    ws = torch.full(((need + 3) // 4 + 16,), -1, dtype=torch.int32, device=dev)      # no larger than the calls can need
    mx, lse = torch.full((b * 65,), float("nan"), device=dev), torch.full((b * 65,), float("nan"), device=dev)
    af = torch.full((1,), 1, dtype=torch.int32, device=dev)

    def raw(logits=ld, ldx=v, k_=k, v_=v, out_=out, ws_bytes=ws.numel() * 4):
        return lib.nm_beam_topk_step_wide(
            ops._stream(), logits.data_ptr(), ldx, b, k_, v_, lps.data_ptr(), lens.data_ptr(), fin.data_ptr(), pen.data_ptr(), c.end,
            *[None if t is None else t.data_ptr() for t in out_], ws.data_ptr(), ws_bytes, af.data_ptr(),
            mx.data_ptr(), lse.data_ptr(), None, None, None, 0)

    if what == "k0":
        rc = raw(k_=0)
    elif what == "k65":
        rc = raw(k_=65)
    elif what == "kv_2_31":
        rc = raw(k_=64, v_=1 << 25, ldx=1 << 25)                      # refused on the sizes alone: nothing is read
    elif what == "short_workspace":
        assert raw(ws_bytes=need) == 0                                # exactly enough is accepted
        for t, fresh in zip(out, _sentinels(dev, b, 65)):
            t.copy_(fresh)
        af.fill_(1)
        ws.fill_(-1)
        mx.fill_(float("nan"))
        rc = raw(ws_bytes=need - 1)
    elif what == "null_output":
        rc = raw(out_=out[:3] + [None] + out[4:])
    else:
        rc = raw(ldx=v - 1)
    assert rc != 0
    assert b"nm_beam_topk_step_wide" in lib.nm_last_error()
    torch.cuda.synchronize()
    # nothing ran: every output, the flag and the workspace still hold their sentinels
    for n, t in zip(OUTS, out):
        a = t.cpu().numpy()
        assert np.isnan(a).all() if a.dtype == np.float32 else (a == -77).all(), n
    assert int(af.item()) == 1 and bool((ws == -1).all()) and bool(torch.isnan(mx).all())
    with pytest.raises(_lib.NMHipError):
        ops.beam_topk_step_wide(ld, b, k, lps, lens, fin, pen, c.end, *[t[:, :k].contiguous() for t in out],
                                torch.empty(need - 1, dtype=torch.uint8, device=dev), mx, lse)


@pytest.mark.parametrize("k", [1, 4, 8, 16])
def test_narrow_workspace_size_is_unchanged(k):
    from neuralmonkey_amd import _lib
    lib = _lib.load()
    for b, v in ((1, 5), (3, 1000), (128, 32000)):
        assert int(lib.nm_beam_workspace_bytes(b, k, v)) == b * 64 * 16 * 8 + 256
