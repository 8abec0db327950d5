"""Torch-CPU restatement of the multi-head scaled dot-product attention of the reference's
attention/scaled_dot_product.py as the header of neuralmonkey_amd/csrc/nm_sdp_attention.hip describes it: test
infrastructure, CPU only.  Every function takes the dtype it computes in (float64: the expected values; float32: the
unit of the derived GPU tolerances).

    energies = (q / sqrt(dh)) . k^T                         per head, heads are column blocks of the model dim
    [causal]   where(j <= i + Tk - Tq, e, -1e9)
    [key mask] e * m + (1 - m) * -1e9
    w = softmax(e) ; wd = w * dropout_mask ; ctx = wd . v

The dropout mask is the counter-based one of oracle.general_ref.dropout_mask over the flat [Bq, H, Tq, Tk] index of
the weights, salted with ``salt + step * 0x9E3779B9 mod 2^32``.  Query row r reads key batch r // rows_per_key.  The
step form reads position j of row r from cache row ``ancestors[r, j]``.

Besides the arithmetic: ``variant`` (which kernel the library launches for a shape, a labelling aid) and ``forced``
(a library context with NM_SDP_MFMA / NM_SDP_DECODE switched, bound for the duration of a ``with`` block)."""
import contextlib
import ctypes
import math
import os

import torch

from oracle import general_ref as G

LDS_LIMIT = 160 * 1024
MFMA_WIDTHS = (16, 32, 64, 128)


def resalt(salt, step):
    """The salt a kernel uses when its ``step`` device scalar holds ``step`` (nm_sdp.h: sdp_keep)."""
    return (int(salt) + int(step) * 0x9E3779B9) & 0xFFFFFFFF


def gather_cache(cache, ancestors, tk):
    """[R, Tmax, D] cache, [R, >= tk] ancestor table -> [R, tk, D] with out[r, j] = cache[ancestors[r, j], j]."""
    pos = torch.arange(tk)[None, :].expand(cache.shape[0], tk)
    return cache[ancestors[:, :tk].long(), pos]


def attention(q, k, v, mask, heads, causal=False, keep=1.0, salt=0, step=0, rpk=1, dctx=None, ancestors=None,
              dtype=torch.float64):
    """q [Bq, Tq, D], k / v [Bk, Tk, D] (Bq = Bk * rpk), mask [Bk, Tk] of 0 / 1 or None -> dict with ``ctx``
    [Bq, Tq, D] and ``w`` [Bq, H, Tq, Tk] (the softmax output, before dropout) and, when ``dctx`` is given, ``dq``,
    ``dk``, ``dv`` by autograd -- everything computed in ``dtype`` on the CPU.  With ``ancestors`` ([Bq, >= Tk] int)
    k / v are the first Tk positions of the caches, [Bq, Tk, D], read through the table (rpk must be 1)."""
    q, k, v = (x.detach().cpu().to(dtype).requires_grad_(dctx is not None) for x in (q, k, v))
    bq, tq, d = q.shape
    dh = d // heads
    kk, vv = k, v
    if ancestors is not None:
        assert rpk == 1
        kk, vv = gather_cache(k, ancestors.cpu(), k.shape[1]), gather_cache(v, ancestors.cpu(), v.shape[1])
    tk = kk.shape[1]
    split = lambda x: x.view(x.shape[0], x.shape[1], heads, dh).permute(0, 2, 1, 3)
    qq = split(q * (1.0 / math.sqrt(dh)))
    kh = split(kk).repeat_interleave(rpk, 0)
    vh = split(vv).repeat_interleave(rpk, 0)
    e = qq @ kh.transpose(-1, -2)
    if causal:
        i = torch.arange(tq)[:, None]
        j = torch.arange(tk)[None, :]
        e = torch.where(j <= i + tk - tq, e, torch.full_like(e, -1e9))
    if mask is not None:
        m4 = mask.detach().cpu().to(dtype)[:, :tk].repeat_interleave(rpk, 0)[:, None, None, :]
        e = e * m4 + (1 - m4) * -1e9
    w = torch.softmax(e, -1)
    wd = w
    if keep < 1.0:
        drop = G.dropout_mask(w.numel(), keep, resalt(salt, step))          # float32 0 or 1 / keep, as the kernels'
        wd = w * torch.from_numpy(drop).to(dtype).view(w.shape)
    ctx = (wd @ vh).permute(0, 2, 1, 3).reshape(bq, tq, d)
    out = {"ctx": ctx.detach(), "w": w.detach()}
    if dctx is not None:
        ctx.backward(dctx.detach().cpu().to(dtype))
        out.update(dq=q.grad, dk=k.grad, dv=v.grad)
    return out


# ------------------------------------------------------------------------------------------- dispatch
def fwd_lds(tk, dh):
    """sdp_fwd_lds (nm_sdp_attention.hip): bytes of LDS the wave-per-query forward takes."""
    return 4 * (2 * tk * (dh + 1) + tk + 4 * dh + 4 * tk)


def bwd_lds(tq, tk, dh):
    """nm_sdp_attn_bwd: (bytes without, bytes with the [Tq, Tk] energy-gradient and weight matrices in LDS)."""
    lds = 4 * (2 * (tk + tq) * (dh + 1) + tk + 4 * tk)
    return lds, lds + 4 * 2 * tq * (tk + 1)


def bwd_mfma_lds(nt, ndt):
    """sdp_bwd_mfma_lds<NT, NDT> (nm_sdp_mfma.hip)."""
    return 4 * 16 * nt * (2 * (16 * ndt + 4) + (16 * nt + 4) + 1)


def _tiles(t):
    return 2 if t <= 32 else 4 if t <= 64 else 8


def _decode_ok(tq, dh, aligned):
    return tq == 1 and dh % 4 == 0 and 64 % (dh // 4) == 0 and dh <= 256 and aligned


def variant(kind, Tq, Tk, H, dh, rpk=1, aligned=True, mfma_on=True, decode_on=True):
    """Which kernel the library launches for a shape: ("mfma", NKT or NT, NDT), ("decode", LPK), ("scalar",),
    ("scalar_bwd", wlds) or ("refused",).  ``kind`` is "fwd", "bwd" or "step"; ``aligned`` says that every operand
    starts on 16 bytes and has a batch stride that is a multiple of 4 floats.

    A LABELLING AID, not a specification: a pure-Python copy of the dispatch rules, so that the tests can say which
    kernel a case is meant for and check that their case list reaches every one.  It mirrors
      * nm_sdp_attn_fwd / nm_sdp_attn_step / nm_sdp_attn_bwd and sdp_decode_launch in csrc/nm_sdp_attention.hip (the
        LDS requirements come first and hold whichever kernel is chosen; nm_sdp_attn_step has no LDS requirement and
        does not look at NM_SDP_DECODE),
      * nm_sdp_mfma_fwd / sdp_fwd_mfma_keys and nm_sdp_mfma_bwd / sdp_bwd_mfma_tiles / sdp_bwd_mfma_launch in
        csrc/nm_sdp_mfma.hip.
    Where the library's choice can be observed (a refusal is an error code; the wave-per-query kernels reproduce
    themselves bit for bit) the tests check the label against the library."""
    vec = aligned and (H * dh) % 4 == 0
    if kind == "step":
        return ("decode", dh // 4) if _decode_ok(1, dh, vec) else ("refused",)
    if kind == "fwd":
        if fwd_lds(Tk, dh) > LDS_LIMIT:
            return ("refused",)
        if mfma_on and Tq >= 8 and Tk <= 128 and vec and dh in MFMA_WIDTHS:
            return ("mfma", _tiles(Tk), dh // 16)
        if decode_on and _decode_ok(Tq, dh, vec):
            return ("decode", dh // 4)
        return ("scalar",)
    assert kind == "bwd", kind
    lds, lds_w = bwd_lds(Tq, Tk, dh)
    if lds > LDS_LIMIT:
        return ("refused",)
    if mfma_on and rpk == 1 and 8 <= Tq <= 128 and Tk <= 128 and vec and dh in MFMA_WIDTHS:
        nt = _tiles(max(Tq, Tk))
        if bwd_mfma_lds(nt, dh // 16) <= LDS_LIMIT:
            return ("mfma", nt, dh // 16)
    return ("scalar_bwd", lds_w <= LDS_LIMIT)


# ------------------------------------------------------------------------------------------- switches
@contextlib.contextmanager
def forced(**switches):
    """``with forced(NM_SDP_MFMA=0):`` -- the calling thread's library calls inside the block run under a context that
    read the given switches.  In order: the variables go into os.environ, nm_create(-1) reads them, nm_ctx_switch
    confirms that it did, nm_ctx_bind binds the context.  On the way out (always): the thread goes back to the default
    context, the context is destroyed and the environment is what it was.  Not nestable; no other thread is affected
    (binding is per thread) unless it creates a context of its own inside the block."""
    from neuralmonkey_amd import _lib
    lib = _lib.load()
    assert all(name in ("NM_SDP_MFMA", "NM_SDP_DECODE") for name in switches), switches
    default = lib.nm_ctx_current()
    saved = {name: os.environ.get(name) for name in switches}
    ctx = ctypes.c_void_p()
    try:
        for name, value in switches.items():
            os.environ[name] = str(int(value))
        assert lib.nm_create(-1, ctypes.byref(ctx)) == 0 and ctx.value, lib.nm_last_error()
        for name, value in switches.items():
            got = ctypes.c_int(12345)
            assert lib.nm_ctx_switch(ctx, name[3:].lower().encode(), ctypes.byref(got)) == 0, lib.nm_last_error()
            assert got.value == int(bool(int(value))), (name, value, got.value)
        assert lib.nm_ctx_bind(ctx) == 0, lib.nm_last_error()
        assert lib.nm_ctx_current() == ctx.value
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
        assert {name: os.environ.get(name) for name in switches} == saved


def err32(ref64, ref32, key):
    """max |float32 CPU restatement - float64| of one output: the unit of a derived bound."""
    return float((ref32[key].double() - ref64[key]).abs().max())
