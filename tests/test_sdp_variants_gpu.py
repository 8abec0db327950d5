"""Every kernel family behind nm_sdp_attn_fwd / nm_sdp_attn_bwd / nm_sdp_attn_step against a float64 restatement of
the operation (tests/sdp_ref.py), at the shapes and under the switches where the dispatch changes kernels:

  A  sdp_bwd_kernel<false>: the scalar backward whose energy gradients go through global memory
  B  sdp_fwd_kernel / sdp_bwd_kernel<true> where the matrix-core or the decode kernel normally runs
     (NM_SDP_MFMA=0, NM_SDP_DECODE=0, an operand off 16-byte alignment)
  C  matrix-core tile edges (sdp_fwd_mfma_kernel<NKT,NDT>, sdp_bwd_mfma_kernel<NT,NDT>)
  D  sdp_decode_kernel<LPK> for every LPK, keys on both sides of an unrolled pass, nm_sdp_attn_step
  E  semantics: an all-zero mask row, fully masked queries, weights=None, the ``step`` scalar, rows_per_key,
     a saturated softmax
  F  (CPU) the case list reaches every kernel instantiation, by tests/sdp_ref.py: variant

Bounds against float64, the ones test_sdp_attention_inside_caches_and_gradient_accumulation holds these kernels to:
weights 2e-6 absolute, ctx 1e-5 * max(|ctx|max, 1), gradients 2e-5 * max(|grad|max, 1).  A case marked ``derived``
(the saturated softmax, whose energies are in the hundreds) adds four times the error of the same computation in
float32 torch on the CPU, the form of test_batch_norm_backward_within_four_times_float32_torch.  Every figure is
printed before it is asserted (pytest -s).  Outputs are NaN-filled before each call and sit inside larger NaN-filled
buffers that must come back untouched."""
import contextlib
import zlib
from typing import NamedTuple, Tuple

import numpy as np
import pytest
import torch

from . import sdp_ref as R

gpu = pytest.mark.gpu
NAN = float("nan")
SALT = 977
MFMA_OFF = (("NM_SDP_MFMA", 0),)
DECODE_OFF = (("NM_SDP_DECODE", 0),)
SCALAR_ONLY = (("NM_SDP_MFMA", 0), ("NM_SDP_DECODE", 0))


class Case(NamedTuple):
    tq: int
    tk: int
    dh: int
    heads: int = 2
    bk: int = 2                  # key batch rows; there are bk * rpk query rows
    causal: bool = False
    masked: bool = True          # a ragged key mask with at least one kept key per row (False: no mask at all)
    keep: float = 1.0
    rpk: int = 1
    env: Tuple = ()              # switches of the context the case runs under
    bwd: bool = True
    accum: bool = False          # check accumulate=True onto a non-zero base as well
    qscale: float = 1.0          # 30: saturated softmax
    zero_row: bool = False       # key batch row 0 has an all-zero mask
    derived: bool = False        # bound = floor + 4 x the float32 CPU restatement's error

    @property
    def ident(self):
        s = "{}x{}x{}-h{}".format(self.tq, self.tk, self.dh, self.heads)
        s += ("-causal" if self.causal else "") + ("" if self.masked else "-nomask")
        s += ("-keep{}".format(self.keep) if self.keep < 1 else "") + ("-rpk{}".format(self.rpk) if self.rpk > 1 else "")
        s += "".join("-{}={}".format(n[3:].lower(), v) for n, v in self.env)
        s += ("-q{}".format(self.qscale) if self.qscale != 1 else "") + ("-zerorow" if self.zero_row else "")
        return s + ("" if self.bwd else "-fwd")

    def label(self, kind, aligned=True):
        env = dict(self.env)
        return R.variant(kind, self.tq, self.tk, self.heads, self.dh, self.rpk, aligned,
                         bool(env.get("NM_SDP_MFMA", 1)), bool(env.get("NM_SDP_DECODE", 1)))


# ------------------------------------------------------------------------------------------- the case lists
A_CASES = [
    Case(129, 129, 64, causal=True, keep=0.9, accum=True),
    Case(130, 130, 32, masked=False),
    Case(70, 70, 128, heads=1),                    # matrix-core forward <8,8>; backward <8,8> declined for LDS
    Case(64, 64, 128, env=MFMA_OFF),               # 166,656 bytes with the matrices in LDS
    Case(140, 140, 16, keep=0.8),
    Case(250, 250, 8),
    Case(150, 150, 64),                            # 159,000 bytes of tiles: close to the largest that is accepted
]
B_MFMA_OFF = [
    Case(12, 12, 64, heads=8, causal=True, keep=0.8, env=MFMA_OFF),
    Case(50, 50, 64, env=MFMA_OFF, accum=True),
    Case(20, 30, 128, env=MFMA_OFF),               # the c += 64 channel loops take a second trip
    Case(33, 17, 64, causal=True, env=MFMA_OFF),
]
B_DECODE_OFF = [
    Case(1, 50, 64, heads=8, rpk=5, env=DECODE_OFF, bwd=False),
    Case(1, 1, 32, env=DECODE_OFF, bwd=False),
    Case(1, 130, 128, env=DECODE_OFF, bwd=False),
    Case(1, 9, 256, heads=20, env=DECODE_OFF, bwd=False),
    Case(1, 23, 4, keep=0.8, env=DECODE_OFF, bwd=False),
]
B_OFF_ALIGNMENT = [Case(12, 12, 64), Case(1, 37, 64, bwd=False)]
C_CASES = [
    Case(8, 1, 64), Case(8, 2, 64, causal=True), Case(15, 16, 64, keep=0.8), Case(16, 16, 64, causal=True),
    Case(17, 33, 64, masked=False), Case(32, 32, 64, causal=True, keep=0.9), Case(63, 64, 64),
    Case(64, 65, 64, causal=True, accum=True), Case(65, 64, 64, keep=0.7), Case(100, 128, 64, causal=True, keep=0.8),
    Case(128, 127, 64, causal=True), Case(127, 128, 64, masked=False, keep=0.9), Case(128, 128, 64, causal=True),
    Case(9, 128, 16, keep=0.8), Case(65, 31, 32, causal=True),
    Case(32, 32, 128, causal=True), Case(64, 64, 128, keep=0.9), Case(16, 128, 128, bwd=False),
    Case(7, 40, 64), Case(8, 40, 64),              # the last scalar and the first matrix-core query count
    Case(129, 40, 64, causal=True),                # three query blocks forward, the scalar kernel backward
    Case(200, 128, 64, bwd=False),                 # four query blocks, the last one partial (backward: refused)
]
D_CASES = (
    [Case(1, tk, 64, heads=h, bwd=False, keep=kp, rpk=rpk)
     for tk, h, kp, rpk in ((3, 1, 1.0, 1), (4, 3, 1.0, 2), (5, 20, 0.8, 1), (15, 3, 1.0, 1), (16, 20, 1.0, 1),
                            (17, 1, 0.9, 3), (33, 3, 1.0, 1))]
    + [Case(1, tk, 4, heads=h, bwd=False, masked=m) for tk, h, m in ((63, 3, True), (64, 20, True), (65, 1, False),
                                                                     (257, 3, True))]
    + [Case(1, tk, 256, heads=h, bwd=False) for tk, h in ((1, 3), (4, 1), (5, 20))]
    + [Case(1, 129, 8, heads=3, bwd=False, keep=0.8), Case(1, 65, 16, heads=20, bwd=False),
       Case(1, 33, 32, heads=1, bwd=False, masked=False), Case(1, 9, 128, heads=3, bwd=False, causal=True)]
)
# one representative per family: matrix cores / decode (its backward: the scalar one, LDS matrices) / scalar with the
# matrices in LDS / scalar forward (Tk > 128) with the backward through global memory
REPS = {"mfma": Case(20, 24, 64), "decode": Case(1, 21, 64), "scalar": Case(5, 21, 8), "global": Case(130, 132, 16)}
E_ZERO_ROW = [c._replace(zero_row=True) for c in REPS.values()]
E_ALL_MASKED = [Case(24, 20, 64, causal=True), Case(7, 5, 8, causal=True), Case(140, 130, 16, causal=True)]
E_STEP = [c._replace(keep=0.8) for c in REPS.values()]
E_RPK = [REPS[n]._replace(rpk=3, bwd=False) for n in ("mfma", "decode", "scalar")]
E_SATURATED = [c._replace(qscale=30.0, derived=True, causal=(n == "mfma")) for n, c in REPS.items()]
E_CASES = E_ZERO_ROW + E_ALL_MASKED + E_STEP + E_RPK + E_SATURATED
ALL_CASES = A_CASES + B_MFMA_OFF + B_DECODE_OFF + B_OFF_ALIGNMENT + C_CASES + D_CASES + E_CASES

ids = lambda cases: [c.ident for c in cases]


# ------------------------------------------------------------------------------------------- inputs and references
class Inputs(NamedTuple):
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    mask: torch.Tensor           # [bk, tk] or None
    g: torch.Tensor              # dctx
    bases: Tuple                 # what accumulate=True adds onto


_INPUTS, _REFS = {}, {}


def _data_key(case):
    return case._replace(env=(), bwd=True, accum=False, derived=False)


def _inputs(case):
    key = _data_key(case)
    if key not in _INPUTS:
        rng = np.random.default_rng(zlib.crc32(repr(tuple(key)).encode()))
        d, bq = case.heads * case.dh, case.bk * case.rpk
        nrm = lambda *shape: torch.tensor(rng.standard_normal(shape).astype(np.float32))
        q, k, v = nrm(bq, case.tq, d) * case.qscale, nrm(case.bk, case.tk, d), nrm(case.bk, case.tk, d)
        g = nrm(bq, case.tq, d)
        mask = None
        if case.masked or case.zero_row:
            m = np.ones((case.bk, case.tk), np.float32)
            if case.masked:
                for i in range(case.bk):
                    m[i, rng.integers(1, case.tk + 1):] = 0
            if case.zero_row:
                m[0] = 0
            mask = torch.tensor(m)
        _INPUTS[key] = Inputs(q, k, v, mask, g, tuple(nrm(*x.shape) for x in (q, k, v)))
    return _INPUTS[key]


def _ref(case, step=0, dtype=torch.float64):
    """The restatement's outputs for a case, computed once and shared (nobody writes into them)."""
    key = (_data_key(case), step, dtype)
    if key not in _REFS:
        x = _inputs(case)
        _REFS[key] = R.attention(x.q, x.k, x.v, x.mask, case.heads, case.causal, case.keep, SALT, step, case.rpk,
                                 dctx=x.g if case.rpk == 1 else None, dtype=dtype)
    return _REFS[key]


def _absmax(t):
    return float(t.abs().max())


def _bounds(case, step=0, add=None):
    """{output: bound} against float64; ``add``: what accumulate=True added onto (the scale is the sum's)."""
    want = dict(_ref(case, step))
    if add:
        want.update({n: want[n] + b.double() for n, b in add.items()})
    out = {"w": 2e-6, "ctx": 1e-5 * max(_absmax(want["ctx"]), 1.0)}
    out.update({n: 2e-5 * max(_absmax(want[n]), 1.0) for n in ("dq", "dk", "dv") if n in want})
    if case.derived:
        r64, r32 = _ref(case, step), _ref(case, step, torch.float32)
        for n in out:
            out[n] += 4.0 * R.err32(r64, r32, n)
    return out


def _close(what, got, want, bound):
    err = float((got.double() - want.double()).abs().max())
    print("{:<60s} err {:.3e}  bound {:.3e}".format(what, err, bound))
    assert err < bound, (what, err, bound)            # (a NaN fails)


# ------------------------------------------------------------------------------------------- running the kernels
def _guarded(x, extra, dev, fill=True):
    """x [B,T,D] as the first T positions of a NaN-filled [B,T+extra,D] device buffer -> (buffer, view, guard)."""
    full = torch.full((x.shape[0], x.shape[1] + extra, x.shape[2]), NAN, device=dev)
    view = full[:, :x.shape[1]]
    if fill:
        view.copy_(x)
    return full, view, full[:, x.shape[1]:]


def _off_alignment(x, dev, fill=True):
    """x [B,T,D] as a contiguous view that starts one float into a NaN-filled flat device buffer."""
    n = x.numel()
    flat = torch.full((n + 8,), NAN, device=dev)
    view = flat[1:1 + n].view(x.shape)
    assert view.data_ptr() % 16 == 4
    if fill:
        view.copy_(x)
    return flat, view, torch.cat((flat[:1], flat[1 + n:]))


class Fwd(NamedTuple):
    ctx: torch.Tensor            # CPU copies
    w: torch.Tensor
    dev: Tuple                   # the device operands, for the backward


def _fwd(dev, case, weights=True, step=None, off=None):
    from neuralmonkey_amd import ops
    x = _inputs(case)
    place = lambda name, t, extra, fill=True: (_off_alignment(t, dev, fill) if off == name
                                               else _guarded(t, extra, dev, fill))
    (_, qd, _), (_, kd, _), (_, vd, _) = place("q", x.q, 2), place("k", x.k, 3), place("v", x.v, 5)
    ctx_full, ctx, ctx_guard = place("ctx", x.q, 3, fill=False)
    mask_wide = None
    if x.mask is not None:
        mask_wide = torch.full((case.bk, case.tk + 4), NAN, device=dev)
        mask_wide[:, :case.tk] = x.mask.to(dev)
    n = x.q.shape[0] * case.heads * case.tq * case.tk
    w_full = torch.full((n + 8,), NAN, device=dev)
    w = w_full[:n].view(x.q.shape[0], case.heads, case.tq, case.tk)
    ops.sdp_attn_fwd(qd, kd, vd, mask_wide, case.heads, ctx, w if weights else None, case.causal, case.rpk, case.keep,
                     SALT, step)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ctx_guard).all()) and bool(torch.isnan(w_full[n:]).all())
    if not weights:
        assert bool(torch.isnan(w_full).all())
    return Fwd(ctx.cpu().clone(), w.cpu().clone(), (qd, kd, vd, mask_wide, w, ctx))


def _bwd(dev, case, fwd, accumulate=False, step=None, off=None):
    """-> {"dq", "dk", "dv"} CPU copies; accumulate=True starts from the case's bases, False from NaN."""
    from neuralmonkey_amd import ops
    x = _inputs(case)
    qd, kd, vd, mask_wide, w = fwd.dev[:5]
    _, gd, _ = _off_alignment(x.g, dev) if off == "dctx" else _guarded(x.g, 1, dev)
    outs, guards = [], []
    for name, t, extra, base in (("dq", x.q, 1, x.bases[0]), ("dk", x.k, 2, x.bases[1]), ("dv", x.v, 4, x.bases[2])):
        _, view, guard = _off_alignment(t, dev, False) if off == name else _guarded(t, extra, dev, False)
        if accumulate:
            view.copy_(base)
        outs.append(view)
        guards.append(guard)
    de = torch.empty((x.q.shape[0], case.heads, case.tq, case.tk), device=dev)
    ops.sdp_attn_bwd(qd, kd, vd, mask_wide, w, gd, case.heads, outs[0], outs[1], outs[2], de, case.causal, case.keep,
                     SALT, accumulate=accumulate, step=step)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(g_).all()) for g_ in guards)
    return {n: o.cpu().clone() for n, o in zip(("dq", "dk", "dv"), outs)}


def _context(case):
    return R.forced(**dict(case.env)) if case.env else contextlib.nullcontext()


def _run(dev, case, step=None, step_value=0):
    """Forward (and backward) of a case under its context, each output checked against float64 -> the outputs."""
    with _context(case):
        fwd = _fwd(dev, case, step=step)
        ref, bound = _ref(case, step_value), _bounds(case, step_value)
        _close(case.ident + " w", fwd.w, ref["w"], bound["w"])
        _close(case.ident + " ctx", fwd.ctx, ref["ctx"], bound["ctx"])
        out = {"ctx": fwd.ctx, "w": fwd.w}
        if case.bwd and case.rpk == 1:
            grads = _bwd(dev, case, fwd, accumulate=False, step=step)
            for n, got in grads.items():
                _close(case.ident + " " + n, got, ref[n], bound[n])
            out.update(grads)
            if case.accum:
                x = _inputs(case)
                add = dict(zip(("dq", "dk", "dv"), x.bases))
                bound = _bounds(case, step_value, add)
                for n, got in _bwd(dev, case, fwd, accumulate=True, step=step).items():
                    _close(case.ident + " base + " + n, got, ref[n] + add[n].double(), bound[n])
    return out


def _default_context_is_current():
    from neuralmonkey_amd import _lib
    lib = _lib.load()
    cur = lib.nm_ctx_current()
    assert lib.nm_ctx_bind(None) == 0 and lib.nm_ctx_current() == cur
    import os
    assert "NM_SDP_MFMA" not in os.environ and "NM_SDP_DECODE" not in os.environ


# ------------------------------------------------------------------------------------------- A
@gpu
@pytest.mark.parametrize("case", A_CASES, ids=ids(A_CASES))
def test_backward_through_global_memory(dev, case):
    """sdp_bwd_kernel<false>: phase 2 reads the energy gradients other waves stored to global memory.

    All of these cases are longer than 128 positions or as wide as dh = 128 and all of them meet the fixed bounds
    (measured on the MI355X: every error below 0.12 of its bound; the float32 CPU restatement itself is within
    2.4e-7 of float64 in the weights and 3.8e-6 in the gradients here), so none is marked ``derived``."""
    assert case.label("bwd") == ("scalar_bwd", False)
    _run(dev, case)
    _default_context_is_current()


# ------------------------------------------------------------------------------------------- B
@gpu
@pytest.mark.parametrize("case", B_MFMA_OFF + B_DECODE_OFF, ids=ids(B_MFMA_OFF + B_DECODE_OFF))
def test_scalar_kernels_under_a_switch(dev, case):
    """NM_SDP_MFMA=0 / NM_SDP_DECODE=0: sdp_fwd_kernel and sdp_bwd_kernel<true> where the fast kernels normally run;
    the forced and the default-context results also agree with each other within the same bounds."""
    assert case.label("fwd") == ("scalar",) and case._replace(env=()).label("fwd")[0] in ("mfma", "decode")
    if case.bwd:
        assert case.label("bwd") == ("scalar_bwd", True) and case._replace(env=()).label("bwd")[0] == "mfma"
    forced = _run(dev, case)
    _default_context_is_current()
    default = _run(dev, case._replace(env=()))
    bound = _bounds(case)
    for n in forced:
        _close(case.ident + " forced vs default " + n, forced[n], default[n], bound[n])


@gpu
@pytest.mark.parametrize("case", B_OFF_ALIGNMENT, ids=ids(B_OFF_ALIGNMENT))
@pytest.mark.parametrize("operand", ["q", "k", "v", "ctx"])
def test_an_operand_off_16_byte_alignment_takes_the_scalar_kernels(dev, case, operand):
    """One operand starts one float into its buffer: the matrix-core and the decode kernel decline (both load 16 bytes
    at a time), the result still matches float64 -- and is, bit for bit, what the wave-per-query kernels give on
    aligned operands when both fast paths are switched off: the same kernel ran.  nm_sdp_attn_step has no scalar
    kernel behind it and refuses.  Backward (the first shape): the same with q / k / v, the context gradient ("ctx")
    off alignment."""
    from neuralmonkey_amd import _lib, ops
    assert case.label("fwd")[0] in ("mfma", "decode") and case.label("fwd", aligned=False) == ("scalar",)
    ref, bound = _ref(case), _bounds(case)
    off = _fwd(dev, case, off=operand)
    _close(case.ident + " w", off.w, ref["w"], bound["w"])
    _close(case.ident + " ctx", off.ctx, ref["ctx"], bound["ctx"])
    with R.forced(**dict(SCALAR_ONLY)):
        scalar = _fwd(dev, case)
    _default_context_is_current()
    assert torch.equal(off.ctx, scalar.ctx) and torch.equal(off.w, scalar.w)
    if case.tq == 1:
        qd, kd, vd, mask_wide, w, ctx = off.dev
        anc = torch.arange(qd.shape[0], dtype=torch.int32, device=dev)[:, None].expand(-1, case.tk).contiguous()
        assert case.label("step", aligned=False) == ("refused",)
        with pytest.raises(_lib.NMHipError, match="16-byte aligned"):
            ops.sdp_attn_step(qd, kd, vd, mask_wide, case.heads, anc, ctx, w)
        return
    assert case.label("bwd")[0] == "mfma" and case.label("bwd", aligned=False) == ("scalar_bwd", True)
    off_b = "dctx" if operand == "ctx" else None
    grads = _bwd(dev, case, off, off=off_b)
    with R.forced(**dict(SCALAR_ONLY)):
        grads_scalar = _bwd(dev, case, scalar)
    for n in grads:
        _close(case.ident + " " + n, grads[n], ref[n], bound[n])
        assert torch.equal(grads[n], grads_scalar[n]), n
    if operand != "ctx":                               # a gradient buffer off alignment declines just the same
        grads = _bwd(dev, case, scalar, off="d" + operand)
        assert all(torch.equal(grads[n], grads_scalar[n]) for n in grads)
    _default_context_is_current()


# ------------------------------------------------------------------------------------------- C
@gpu
@pytest.mark.parametrize("case", C_CASES, ids=ids(C_CASES))
def test_matrix_core_tile_edges(dev, case):
    """Positions at 8, 15 / 16 / 17, 63 / 64 / 65, 127 / 128 and every (NKT, NDT) / (NT, NDT) the suite did not reach;
    7 against 8 queries (the last scalar, the first matrix-core shape); more than one query block forward with the
    scalar kernel backward."""
    from neuralmonkey_amd import _lib
    want = ("mfma",) if case.tq >= 8 else ("scalar",)
    assert case.label("fwd")[:1] == want
    if (case.tq, case.tk) == (200, 128):               # the backward tiles of this shape do not fit: an error, no launch
        assert case.label("bwd") == ("refused",)
        fwd = _fwd(dev, case)
        with pytest.raises(_lib.NMHipError, match="do not fit LDS"):
            _bwd(dev, case, fwd)
    _run(dev, case)


# ------------------------------------------------------------------------------------------- D
@gpu
@pytest.mark.parametrize("case", D_CASES, ids=ids(D_CASES))
def test_decode_kernel_against_float64(dev, case):
    """sdp_decode_kernel<LPK> for the seven LPK = dh / 4, the key count on both sides of one unrolled pass of
    UN * KPP = 256 / LPK keys, fewer and more heads than the workgroup's 16 waves."""
    assert case.label("fwd") == ("decode", case.dh // 4)
    _run(dev, case)


@gpu
@pytest.mark.parametrize("rows,tk,tmax,heads,dh", [(6, 17, 20, 3, 64), (5, 65, 65, 20, 4)])
def test_step_through_an_ancestor_table_against_float64(dev, rows, tk, tmax, heads, dh):
    """nm_sdp_attn_step with a random ancestor table against the float64 gather-then-attend."""
    from neuralmonkey_amd import ops
    rng = np.random.default_rng(rows * 1000 + tk)
    d = heads * dh
    nrm = lambda *shape: torch.tensor(rng.standard_normal(shape).astype(np.float32))
    q, kc, vc = nrm(rows, 1, d), nrm(rows, tmax, d), nrm(rows, tmax, d)
    anc = torch.tensor(rng.integers(0, rows, (rows, tmax)).astype(np.int32))
    mask = torch.tensor((rng.random((rows, tmax)) < 0.8).astype(np.float32))
    mask[:, 0] = 1.0
    ref = R.attention(q, kc[:, :tk], vc[:, :tk], mask, heads, ancestors=anc)
    kd, vd = kc.to(dev), vc.to(dev)
    ctx_full = torch.full((rows, 3, d), NAN, device=dev)
    w = torch.full((rows, heads, 1, tk), NAN, device=dev)
    ops.sdp_attn_step(q.to(dev), kd[:, :tk], vd[:, :tk], mask.to(dev), heads, anc.to(dev), ctx_full[:, :1], w)
    torch.cuda.synchronize()
    _close("step w", w.cpu(), ref["w"], 2e-6)
    _close("step ctx", ctx_full[:, :1].cpu(), ref["ctx"], 1e-5 * max(_absmax(ref["ctx"]), 1.0))
    assert bool(torch.isnan(ctx_full[:, 1:]).all())


@gpu
def test_step_refuses_exactly_the_head_widths_the_decode_kernel_does_not_take(dev):
    from neuralmonkey_amd import _lib, ops
    for dh in (2, 4, 6, 8, 12, 16, 20, 24, 32, 48, 64, 96, 128, 192, 256, 512):
        q = torch.ones((1, 1, 2 * dh), device=dev)
        kv = torch.ones((1, 2, 2 * dh), device=dev)
        anc = torch.zeros((1, 2), dtype=torch.int32, device=dev)
        ctx = torch.full((1, 1, 2 * dh), NAN, device=dev)
        if R.variant("step", 1, 2, 2, dh) == ("refused",):
            with pytest.raises(_lib.NMHipError, match="nm_sdp_attn_step: dh"):
                ops.sdp_attn_step(q, kv, kv, None, 2, anc, ctx)
            assert bool(torch.isnan(ctx).all())
        else:
            ops.sdp_attn_step(q, kv, kv, None, 2, anc, ctx)
            assert float((ctx - 1.0).abs().max()) < 1e-6            # the mean of two rows of ones


# ------------------------------------------------------------------------------------------- E
@gpu
@pytest.mark.parametrize("case", E_ZERO_ROW, ids=ids(E_ZERO_ROW))
def test_an_all_zero_mask_row(dev, case):
    """Every key of batch row 0 is masked: its energies are all -1e9, the weights uniform; no gradient reaches the
    energies (dq and dk of the row are exactly zero) while dv, which does not pass through them, is not."""
    out = _run(dev, case)
    w0 = out["w"][0]
    assert torch.equal(w0.max(-1).values, w0.min(-1).values)
    assert float((w0 - 1.0 / case.tk).abs().max()) < 2e-6
    assert bool((out["dq"][0] == 0).all()) and bool((out["dk"][0] == 0).all())
    assert _absmax(out["dv"][0]) > 0.01


@gpu
@pytest.mark.parametrize("case", E_ALL_MASKED, ids=ids(E_ALL_MASKED))
def test_queries_with_every_key_in_the_future(dev, case):
    """Causal with more queries than keys: the first Tq - Tk queries see no key at all -- uniform weights over all Tk
    keys (the key mask cannot tell -1e9 from -1e9) and a zero energy gradient, so their dq is exactly zero.  These
    rows are the only place where the backward kernels' "tf.where passes no gradient" rule can be seen at all: a
    masked key of any other query has a weight of exactly zero, and with it a zero softmax gradient."""
    out = _run(dev, case)
    dead = case.tq - case.tk
    w = out["w"][:, :, :dead]
    assert torch.equal(w.max(-1).values, w.min(-1).values)
    assert float((w - 1.0 / case.tk).abs().max()) < 2e-6
    assert bool((out["dq"][:, :dead] == 0).all())


@gpu
@pytest.mark.parametrize("name", sorted(REPS))
def test_forward_without_a_weights_buffer(dev, name):
    """weights=None: the same ctx bit for bit (under dropout too), nothing written anywhere else."""
    case = REPS[name]._replace(keep=0.8)
    assert torch.equal(_fwd(dev, case, weights=False).ctx, _fwd(dev, case).ctx)


@gpu
@pytest.mark.parametrize("case", E_STEP, ids=ids(E_STEP))
def test_the_step_scalar_resalts_the_dropout_mask(dev, case):
    """``step`` (a device scalar): the mask's salt becomes salt + step * 0x9E3779B9, forward and backward alike.
    step = 0 is no step, bit for bit; step = 3 is another mask, the float64 restatement's with the same salt."""
    none = _run(dev, case)
    zero = _run(dev, case, step=torch.tensor([0], dtype=torch.int32, device=dev), step_value=0)
    three = _run(dev, case, step=torch.tensor([3], dtype=torch.int32, device=dev), step_value=3)
    for n in none:
        assert torch.equal(none[n], zero[n]), n
    assert torch.equal(none["w"], three["w"])                      # the softmax output is saved before the dropout
    for n in ("ctx", "dq", "dk", "dv"):
        assert not torch.equal(none[n], three[n]), n


@gpu
@pytest.mark.parametrize("case", E_RPK + E_SATURATED, ids=ids(E_RPK + E_SATURATED))
def test_rows_per_key_and_a_saturated_softmax(dev, case):
    """rows_per_key = 3 (query row r reads key batch r // 3), forward.  Queries scaled by 30: energies in the hundreds,
    weights close to one-hot; the bound of every output is the fixed one plus four times the float32 CPU
    restatement's error, computed per case and printed.  That error (w / ctx / dq / dk / dv) and, in brackets, the
    largest ratio of a kernel's error to its bound as measured on the MI355X:
      20 x 24 x 64 causal   2.3e-6 / 7.4e-6 / 4.3e-6 / 7.4e-5 / 6.3e-6   (0.14)
      1 x 21 x 64           1.2e-6 / 3.4e-6 / 3.1e-7 / 6.9e-6 / 3.0e-6   (0.08)
      5 x 21 x 8            3.9e-7 / 7.9e-7 / 3.7e-7 / 1.2e-5 / 4.5e-7   (0.11)
      130 x 132 x 16        4.1e-6 / 1.1e-5 / 1.2e-5 / 1.6e-4 / 8.2e-6   (0.22)"""
    if case.derived:
        r64, r32 = _ref(case), _ref(case, dtype=torch.float32)
        print(case.ident, "float32 CPU error:", {n: "{:.2e}".format(R.err32(r64, r32, n)) for n in r64})
    _run(dev, case)


# ------------------------------------------------------------------------------------------- F
def test_the_case_list_reaches_every_kernel_instantiation():
    """(CPU) By sdp_ref.variant, the cases above launch every template instantiation of the six kernel families."""
    fwd = {c.label("fwd") for c in ALL_CASES}
    bwd = {c.label("bwd") for c in ALL_CASES if c.bwd and c.rpk == 1}
    assert {(8, 4), (8, 8)} <= {v[1:] for v in fwd if v[0] == "mfma"}
    assert {v[1] for v in fwd if v[0] == "mfma"} == {2, 4, 8} and {v[2] for v in fwd if v[0] == "mfma"} == {1, 2, 4, 8}
    assert {v[1] for v in fwd if v[0] == "decode"} == {1, 2, 4, 8, 16, 32, 64}
    assert {c.dh for c in ALL_CASES if c.label("fwd") == ("scalar",)} >= {64, 128}
    assert {v[1] for v in bwd if v[0] == "mfma"} == {2, 4, 8} and {v[2] for v in bwd if v[0] == "mfma"} == {1, 2, 4, 8}
    assert {(8, 4), (4, 8)} <= {v[1:] for v in bwd if v[0] == "mfma"}
    assert {("scalar_bwd", True), ("scalar_bwd", False)} <= bwd
    assert {c.dh for c in ALL_CASES if c.bwd and c.label("bwd") == ("scalar_bwd", True)} >= {64, 128}
    assert ("refused",) not in fwd and ("refused",) not in bwd
    # the labels the issue's figures pin: LDS bytes by the library's own formulas
    assert R.bwd_lds(129, 129, 64)[1] == 270900 and R.bwd_lds(70, 70, 128)[1] == 185640
    assert R.bwd_lds(70, 130, 32)[1] == 128760 and R.bwd_lds(64, 64, 128)[1] == 166656
    assert R.bwd_lds(150, 150, 64)[0] == 159000 and R.bwd_lds(79, 79, 128)[0] == 164636
    assert R.bwd_mfma_lds(8, 8) == 203264
    # the edges INTEGRATION.md states
    assert R.variant("bwd", 78, 78, 2, 128) != ("refused",) and R.variant("bwd", 79, 79, 2, 128) == ("refused",)
    assert R.variant("bwd", 154, 154, 2, 64) != ("refused",) and R.variant("bwd", 155, 155, 2, 64) == ("refused",)
    assert R.variant("fwd", 1, 301, 2, 64) != ("refused",) and R.variant("fwd", 1, 302, 2, 64) == ("refused",)
    assert R.variant("fwd", 128, 128, 2, 128) == ("mfma", 8, 8)
