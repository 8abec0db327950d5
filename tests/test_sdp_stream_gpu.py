"""The streaming attention kernels (csrc/nm_sdp_stream.hip) on the MI355X against the float64 restatement of
tests/sdp_ref.py: the entry points called directly at the smallest shapes where a tile, a ring stage or the online
softmax can go wrong, then autodiff.sdp_attention at two shapes the resident kernels refuse.

Bounds, as tests/test_sdp_variants_gpu.py: _bounds: weights 2e-6, ctx 1e-5 * max(|ctx|max, 1), gradients
2e-5 * max(|grad|max, 1), each plus four times the error of the float32 CPU restatement.  Every figure is printed
before it is asserted (pytest -s)."""
from typing import NamedTuple

import numpy as np
import pytest
import torch

from . import sdp_ref as R

gpu = pytest.mark.gpu
NAN = float("nan")
SALT, STEP, BK = 977, 3, 3


class Case(NamedTuple):
    tq: int
    tk: int
    dh: int
    heads: int = 2
    causal: bool = False
    mask: str = ""               # "ragged": prefix lengths tk, 5, tk // 2 + 1; "jump": 70 zeros then ones, all zeros, a prefix
    keep: float = 1.0            # below 1: with the step scalar set to STEP
    rpk: int = 1                 # above 1: forward only
    accum: bool = False
    pad: int = 0                 # extra positions between the key / value batch rows
    weights: bool = False
    stats: bool = True           # False: no row_max / row_sum (Tq == 1, keep 1: the one-query kernel runs)

    @property
    def ident(self):
        return "-".join(str(x) for x in self)


CASES = [
    Case(17, 65, 64, causal=True, mask="ragged", keep=0.7, weights=True),
    Case(64, 64, 64, heads=3, accum=True),
    Case(65, 130, 64, mask="jump", weights=True, pad=3),
    Case(70, 200, 64, causal=True, mask="ragged", keep=0.7, accum=True, pad=5),
    Case(33, 129, 16, heads=3, causal=True, mask="jump"),
    Case(33, 129, 128, mask="ragged", keep=0.7, weights=True),
    Case(1, 129, 64, heads=3, mask="ragged", rpk=3, weights=True, stats=False),
    Case(1, 129, 64, mask="jump", keep=0.7, weights=True),
    Case(17, 65, 64, mask="ragged", rpk=3, weights=True),
]


def _mask(kind, tk):
    m = np.ones((BK, tk), np.float32)
    if kind == "ragged":
        m[1, 5:] = 0
        m[2, tk // 2 + 1:] = 0
    else:
        m[0, :70] = 0            # the whole first tile: the running maximum jumps from -1e9 to a real energy
        m[1] = 0                 # fully masked: uniform weights over all tk keys
        m[2, tk - 7:] = 0
    return torch.tensor(m)


def _bounds(ref, ref32, add=None):
    want = dict(ref)
    if add:
        want.update({n: want[n] + b.double() for n, b in add.items()})
    out = {"w": 2e-6, "ctx": 1e-5 * max(float(want["ctx"].abs().max()), 1.0)}
    out.update({n: 2e-5 * max(float(want[n].abs().max()), 1.0) for n in ("dq", "dk", "dv") if n in want})
    return {n: b + 4.0 * R.err32(ref, ref32, n) for n, b in out.items()}


def _close(what, got, want, bound):
    err = float((got.double().cpu() - want.double()).abs().max())
    print("{:<50s} err {:.3e}  bound {:.3e}".format(what, err, bound))
    assert err < bound, (what, err, bound)            # (a NaN fails)


@gpu
@pytest.mark.parametrize("case", CASES, ids=[c.ident for c in CASES])
def test_streaming_kernels_against_float64(dev, case):
    from neuralmonkey_amd import ops
    rng = np.random.default_rng(case.tq * 1000 + case.tk + case.dh)
    d, bq = case.heads * case.dh, BK * case.rpk
    nrm = lambda *shape: torch.tensor(rng.standard_normal(shape).astype(np.float32))
    q, k, v, g = nrm(bq, case.tq, d), nrm(BK, case.tk, d), nrm(BK, case.tk, d), nrm(bq, case.tq, d)
    mask = _mask(case.mask, case.tk) if case.mask else None
    step = STEP if case.keep < 1 else 0
    dctx = g if case.rpk == 1 else None
    ref, ref32 = (R.attention(q, k, v, mask, case.heads, case.causal, case.keep, SALT, step, case.rpk, dctx, dtype=t)
                  for t in (torch.float64, torch.float32))
    bound = _bounds(ref, ref32)

    def cache(x):                                       # the first tk positions of a longer NaN-filled buffer
        full = torch.full((BK, case.tk + case.pad, d), NAN, device=dev)
        full[:, :case.tk] = x.to(dev)
        return full[:, :case.tk]
    qd, kd, vd, gd = q.to(dev), cache(k), cache(v), g.to(dev)
    md = mask.to(dev) if mask is not None else None
    sd = torch.tensor([STEP], dtype=torch.int32, device=dev) if case.keep < 1 else None
    ctx = torch.full_like(qd, NAN)
    w = torch.full((bq, case.heads, case.tq, case.tk), NAN, device=dev) if case.weights else None
    rmax, rsum = (torch.full((bq, case.heads, case.tq), NAN, device=dev) for _ in range(2)) if case.stats else (None, None)
    ops.sdp_stream_fwd(qd, kd, vd, md, case.heads, ctx, w, rmax, rsum, case.causal, case.rpk, case.keep, SALT, sd)
    _close(case.ident + " ctx", ctx, ref["ctx"], bound["ctx"])
    if w is not None:
        _close(case.ident + " w", w, ref["w"], bound["w"])
    if case.rpk > 1 or not case.stats:
        return
    ws = ops.sdp_stream_workspace(bq, case.heads, case.tq, dev)
    bases = {n: nrm(*x.shape) for n, x in (("dq", q), ("dk", k), ("dv", v))}

    def backward(accumulate):
        outs = {n: (b.to(dev) if accumulate else torch.full_like(b, NAN, device=dev)) for n, b in bases.items()}
        ws.fill_(NAN)
        ops.sdp_stream_bwd(qd, kd, vd, md, ctx, rmax, rsum, gd, case.heads, outs["dq"], outs["dk"], outs["dv"], ws,
                           case.causal, case.keep, SALT, accumulate, sd)
        return outs
    first, second = backward(False), backward(False)
    for n in first:
        _close(case.ident + " " + n, first[n], ref[n], bound[n])
        assert torch.equal(first[n], second[n]), n      # no atomics: bit-equal run to run
    if case.accum:
        bound = _bounds(ref, ref32, bases)
        for n, got in backward(True).items():
            _close(case.ident + " base + " + n, got, ref[n] + bases[n].double(), bound[n])


@gpu
@pytest.mark.parametrize("recording", [True, False])
def test_sdp_attention_past_the_resident_kernels_lds_bound(dev, recording):
    """autodiff.sdp_attention where nm_sdp_attn_bwd (160 x 160 x 64, recording) and nm_sdp_attn_fwd (1 x 320 x 64 with
    rows_per_key = 2 and a weights history, not recording) refuse."""
    from neuralmonkey_amd import autodiff as F
    from .tape_ref import PoisonCtx, seed_grad
    heads, dh = 2, 64
    bk, rpk, tq, tk, causal = (2, 1, 160, 160, True) if recording else (2, 2, 1, 320, False)
    bq, d = bk * rpk, heads * dh
    rng = np.random.default_rng(160 + tk)
    nrm = lambda *shape: torch.tensor(rng.standard_normal(shape).astype(np.float32))
    q, k, v, g = nrm(bq, tq, d), nrm(bk, tk, d), nrm(bk, tk, d), nrm(bq, tq, d)
    mask = torch.ones(bk, tk)
    mask[1, tk - 30:] = 0
    ref, ref32 = (R.attention(q, k, v, mask, heads, causal, rpk=rpk, dctx=g if recording else None, dtype=t)
                  for t in (torch.float64, torch.float32))
    bound = _bounds(ref, ref32)
    tape = F.Tape(PoisonCtx(dev), "sdp_stream", recording=recording)
    qv, kv, vv = (tape.leaf(x.reshape(-1, d).to(dev), needs_grad=True) for x in (q, k, v))
    w_out = None if recording else torch.full((bq, heads, tq, tk), NAN, device=dev)
    out = F.sdp_attention(tape, qv, kv, vv, mask.to(dev), heads, bq, tq, bk, tk, causal=causal, w_out=w_out)
    _close("ctx", out.data.view(bq, tq, d), ref["ctx"], bound["ctx"])
    if not recording:
        _close("w", w_out, ref["w"], bound["w"])
        return
    seed_grad(out, g.reshape(-1, d).to(dev))
    tape.backward()
    for n, var, like in (("dq", qv, q), ("dk", kv, k), ("dv", vv, v)):
        _close(n, var.grad.view(like.shape), ref[n], bound[n])
