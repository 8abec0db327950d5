"""Thin Python wrappers over the C-ABI: torch tensors in, HIP kernels out.

torch is used only as the device allocator and stream owner; every arithmetic
op on the hot path is a libnmhip kernel launched on torch's current stream.
"""
import ctypes
import struct
import os
import threading
from typing import Optional

import numpy as np
import torch

from . import _lib

ACT = {None: 0, "none": 0, "tanh": 1, "relu": 2}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _f32(t):
    assert t.dtype == torch.float32 and t.is_cuda, (t.dtype, t.device)
    return t


def _i32(t):
    assert t.dtype == torch.int32 and t.is_cuda, (t.dtype, t.device)
    return t


def add_layer_norm_fwd(a, x, gamma, beta, sum_out, out, eps=1e-6):
    """sum_out = a + x ; out = layer_norm(sum_out) over the last dimension (contiguous [rows, D] operands)."""
    lib = _lib.load()
    d = x.shape[-1]
    rows = x.numel() // d
    assert a.is_contiguous() and x.is_contiguous() and sum_out.is_contiguous() and out.is_contiguous()
    assert a.numel() == x.numel() == sum_out.numel() == out.numel()
    _lib.check(lib.nm_add_layer_norm_fwd(_stream(), a.data_ptr(), d, x.data_ptr(), d, gamma.data_ptr(),
                                         beta.data_ptr(), sum_out.data_ptr(), d, out.data_ptr(), d, rows, d, float(eps)),
               "nm_add_layer_norm_fwd")
    return sum_out, out


def add_layer_norm_stats_ok(a, x, gamma, beta) -> bool:
    """Can ``add_layer_norm_stats_fwd`` take these operands (contiguous rows of D <= 2048 floats, D % 4 == 0, aligned)?"""
    d = x.shape[-1]
    return (x.is_cuda and d % 4 == 0 and d <= 2048 and a.is_contiguous() and x.is_contiguous() and a.shape == x.shape
            and all(t.data_ptr() % 16 == 0 for t in (a, x, gamma, beta)))


def add_layer_norm_stats_fwd(a, x, gamma, beta, sum_out, out, mean, rstd, eps=1e-6):
    """sum_out = a + x ; out = layer_norm(sum_out), with the row statistics the backward pass reads
    (nm_add_layer_norm_stats_fwd: one wave per row)."""
    d = x.shape[-1]
    rows = x.numel() // d
    assert sum_out.is_contiguous() and out.is_contiguous()
    _lib.check(_lib.load().nm_add_layer_norm_stats_fwd(_stream(), a.data_ptr(), x.data_ptr(), gamma.data_ptr(),
                                                       beta.data_ptr(), sum_out.data_ptr(), out.data_ptr(),
                                                       mean.data_ptr(), rstd.data_ptr(), rows, d, float(eps)),
               "nm_add_layer_norm_stats_fwd")
    return sum_out, out


GEMM_BACKGROUND = 4     # nm_gemm_f32 algo: residency-capped 128x128 tiles for a long leaf GEMM on a side stream


def gemm(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None, bias=None, act=None,
         trans_a=False, trans_b=False, accumulate=False, algo=0):
    """out[M,N] = act(op(a) @ op(b) + bias (+ out)).  2-D (or batched 3-D with
    equal leading dim) row-major views with unit inner stride."""
    lib = _lib.load()
    _f32(a), _f32(b)
    batched = a.dim() == 3
    if batched:
        assert b.dim() == 3 and a.shape[0] == b.shape[0]
        nb = a.shape[0]
        a2, b2 = a[0], b[0]
        s_a, s_b = a.stride(0), b.stride(0)
    else:
        nb, a2, b2, s_a, s_b = 1, a, b, 0, 0
    assert a2.stride(1) == 1 and b2.stride(1) == 1, "inner stride must be 1"
    m, k = (a2.shape[1], a2.shape[0]) if trans_a else (a2.shape[0], a2.shape[1])
    kb, n = (b2.shape[1], b2.shape[0]) if trans_b else (b2.shape[0], b2.shape[1])
    assert k == kb, f"inner dims differ: {k} vs {kb}"
    if out is None:
        assert not accumulate
        out = torch.empty((nb, m, n) if batched else (m, n), dtype=torch.float32, device=a.device)
    o2 = out[0] if batched else out
    assert tuple(o2.shape) == (m, n) and o2.stride(1) == 1
    s_c = out.stride(0) if batched else 0
    ws = _gemm_workspace(a.device) if (nb == 1 and k >= 1024) else None
    _lib.check(lib.nm_gemm_f32(_stream(), int(trans_a), int(trans_b), m, n, k,
                               a.data_ptr(), a2.stride(0), b.data_ptr(), b2.stride(0),
                               out.data_ptr(), o2.stride(0), _p(bias), ACT[act], int(accumulate),
                               nb, s_a, s_b, s_c, algo, _p(ws), ws.numel() * 4 if ws is not None else 0),
               "nm_gemm_f32")
    return out


_GROUP_TABLES = {}


def gemm_group(items, trans_a=False, trans_b=False, accumulate=True):
    """``items`` = [(a, b, out)] of ONE shape: out_i (+)= op(a_i) @ op(b_i) in one launch (nm_gemm_f32_group).  The
    device table of operand pointers is built once per distinct list of pointers and kept (a training step names the
    same persistent buffers every time; a captured step replays the launch with its table)."""
    lib = _lib.load()
    a0, b0, o0 = items[0]
    m, k = (a0.shape[1], a0.shape[0]) if trans_a else (a0.shape[0], a0.shape[1])
    n = b0.shape[0] if trans_b else b0.shape[1]
    lda, ldb, ldc = a0.stride(0), b0.stride(0), o0.stride(0)
    ptrs = []
    for a, b, o in items:
        assert a.shape == a0.shape and b.shape == b0.shape and o.shape == o0.shape
        assert (a.stride(0), b.stride(0), o.stride(0)) == (lda, ldb, ldc) and a.stride(1) == b.stride(1) == o.stride(1) == 1
        assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0 and o.data_ptr() % 16 == 0
        ptrs += [a.data_ptr(), b.data_ptr(), o.data_ptr()]
    assert len({p for p in ptrs[2::3]}) == len(items), "two products of a group share their output"
    table = _pointer_table(a0.device, ptrs)
    _lib.check(lib.nm_gemm_f32_group(_stream(), int(trans_a), int(trans_b), m, n, k, table.data_ptr(), lda, ldb, ldc,
                                     int(accumulate), len(items)), "nm_gemm_f32_group")


def _pointer_table(device, ptrs):
    key = (device, tuple(ptrs))
    table = _GROUP_TABLES.get(key)
    if table is None:
        if len(_GROUP_TABLES) > 1024:
            _GROUP_TABLES.clear()
        table = _GROUP_TABLES[key] = torch.tensor(ptrs, dtype=torch.int64, device=device)
    return table


def gemm_chain(members, out, accumulate=True):
    """``out (+)= sum_i a_i^T @ b_i`` over ``members`` = [(a_i, b_i)] of one shape ([rows, M] and [rows, N]) as ONE product
    whose K dimension is the chain of the members (nm_gemm_f32_chain): the weight gradient of a taped time loop."""
    lib = _lib.load()
    a0, b0 = members[0]
    rows, m, n = a0.shape[0], a0.shape[1], b0.shape[1]
    lda, ldb = a0.stride(0), b0.stride(0)
    ptrs = []
    for a, b in members:
        assert a.shape == a0.shape and b.shape == b0.shape and (a.stride(0), b.stride(0)) == (lda, ldb)
        assert a.stride(1) == 1 and b.stride(1) == 1 and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
        ptrs += [a.data_ptr(), b.data_ptr(), 0]
    assert out.shape == (m, n) and out.stride(1) == 1
    table = _pointer_table(a0.device, ptrs)
    ws = _gemm_workspace(a0.device)
    _lib.check(lib.nm_gemm_f32_chain(_stream(), m, n, rows, len(members), table.data_ptr(), lda, ldb, out.data_ptr(),
                                     out.stride(0), int(accumulate), ws.data_ptr(), ws.numel() * 4), "nm_gemm_f32_chain")
    return out


OUTER_CHAIN_MAX = 64


def outer_chain(members, out, accumulate=True):
    """``out[b, s, c] (+)= sum_t w_t[b, s] * d_t[b, c]`` over ``members`` = [(w_t [B, >=S], d_t [B, C])] (nm_outer_chain);
    ``out`` [B, S, C] contiguous."""
    w0, d0 = members[0]
    bsz, s, c = out.shape
    assert out.is_contiguous() and len(members) <= OUTER_CHAIN_MAX
    ptrs = []
    for w, d in members:
        assert w.shape[0] == bsz and d.shape == (bsz, c) and w.stride(1) == 1 and d.stride(1) == 1
        assert w.stride(0) == w0.stride(0) and d.stride(0) == d0.stride(0) and w.shape[1] >= s
        ptrs += [w.data_ptr(), d.data_ptr()]
    table = _pointer_table(out.device, ptrs)
    _lib.check(_lib.load().nm_outer_chain(_stream(), table.data_ptr(), len(members), bsz, s, c, w0.stride(0), d0.stride(0),
                                          out.data_ptr(), int(accumulate)), "nm_outer_chain")
    return out


def colsum_chain(members, out, accumulate=True):
    """``out[c] (+)= sum_i sum_r x_i[r, c]`` over tensors of one shape (nm_colsum_chain): a bias gradient of a taped time
    loop in one launch."""
    lib = _lib.load()
    x0 = members[0]
    rows, cols, ld = x0.shape[0], x0.shape[1], x0.stride(0)
    for x in members:
        assert x.shape == x0.shape and x.stride(0) == ld and x.stride(1) == 1 and x.data_ptr() % 16 == 0
    table = _pointer_table(x0.device, [x.data_ptr() for x in members])
    ws = _colsum_workspace(x0.device, cols)
    _lib.check(lib.nm_colsum_chain(_stream(), table.data_ptr(), 1, 0, len(members), rows, ld, cols, out.data_ptr(),
                                   int(accumulate), ws.data_ptr(), ws.numel() * 4), "nm_colsum_chain")
    return out


_GEMM_WS = {}
GEMM_WORKSPACE_BYTES = 128 << 20
# Scratch that kernels re-use from call to call (split-K slabs, column-sum partials + tickets) is keyed by the stream
# the launch goes to -- but every torch.cuda.graph capture uses torch's ONE capture stream, so two captured graphs
# would share a workspace and may later replay on different streams at the same time (a look-ahead encoder graph
# next to the running batch's decoding graphs).  Whoever captures work for a second stream sets a tag
# (runtime.Session._run_ahead): tagged launches get workspaces of their own.  The tag is per THREAD, like the library's
# context (nm_cur()): another session launching from another thread (the input pipeline's prefetcher, an ensemble's
# sessions) keeps its own.
_TLS = threading.local()


def workspace_tag():
    return getattr(_TLS, "workspace_tag", None)


def set_workspace_tag(tag):
    """Sets this thread's tag; returns the previous one (to be restored by the caller)."""
    old = workspace_tag()
    _TLS.workspace_tag = tag
    return old


def _gemm_workspace(device):
    """Persistent split-K slab buffer, one per (device, stream, tag): kernels of one
    stream are ordered, kernels of different streams must not share slabs."""
    key = (device, _stream(), workspace_tag())
    ws = _GEMM_WS.get(key)
    if ws is None:
        ws = torch.empty(GEMM_WORKSPACE_BYTES // 4, dtype=torch.float32, device=device)
        _GEMM_WS[key] = ws
    return ws


def embedding_gather(table, ids, out=None, mask_pad=False, scale=1.0):
    lib = _lib.load()
    _f32(table), _i32(ids)
    n = ids.numel()
    e = table.shape[1]
    if out is None:
        out = torch.empty(tuple(ids.shape) + (e,), dtype=torch.float32, device=table.device)
    ldo = out.stride(-2) if out.dim() >= 2 else e
    _lib.check(lib.nm_embedding_gather(_stream(), table.data_ptr(), table.shape[0], e,
                                       ids.data_ptr(), n, out.data_ptr(), ldo, int(mask_pad),
                                       float(scale)), "nm_embedding_gather")
    return out


def _rev_mask(ndir, reverse_dir0):
    """bit d set -> direction d walks its sequence backwards (reverse_sequence)."""
    return 1 if reverse_dir0 else (2 if ndir == 2 else 0)


def gru_gates_fwd(xp, x_dir_off, x_row_stride, x_time_stride, hg, h, ru, rh, lengths, t, ndir, rows, hsz,
                  reverse_dir0=False):
    lib = _lib.load()
    _lib.check(lib.nm_gru_gates_fwd(_stream(), xp.data_ptr(), x_dir_off, x_row_stride, x_time_stride,
                                    hg.data_ptr(), h.data_ptr(), ru.data_ptr(), rh.data_ptr(),
                                    _p(lengths), t, _rev_mask(ndir, reverse_dir0), ndir, rows, hsz),
               "nm_gru_gates_fwd")


def gru_blend_fwd(xp, x_dir_off, x_row_stride, x_time_stride, hc, ru, h_in, h_out, c_save, out,
                  out_dir_off, out_row_stride, out_time_stride, lengths, t, ndir, rows, hsz,
                  reverse_dir0=False):
    lib = _lib.load()
    _lib.check(lib.nm_gru_blend_fwd(_stream(), xp.data_ptr(), x_dir_off, x_row_stride, x_time_stride,
                                    hc.data_ptr(), ru.data_ptr(), h_in.data_ptr(), h_out.data_ptr(),
                                    _p(c_save), _p(out), out_dir_off, out_row_stride, out_time_stride,
                                    _p(lengths), t, _rev_mask(ndir, reverse_dir0), ndir, rows, hsz),
               "nm_gru_blend_fwd")


def layer_norm_fwd(x, gamma, beta, out=None, mean=None, rstd=None, eps=1e-6):
    lib = _lib.load()
    d = x.shape[-1]
    rows = x.numel() // d
    assert x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    _lib.check(lib.nm_layer_norm_fwd(_stream(), x.data_ptr(), d, gamma.data_ptr(), beta.data_ptr(),
                                     out.data_ptr(), d, _p(mean), _p(rstd), rows, d, float(eps)),
               "nm_layer_norm_fwd")
    return out


def copy_cols(src, dst):
    """dst[:, :w] = src (2-D views, inner stride 1)."""
    lib = _lib.load()
    assert src.dim() == 2 and dst.dim() == 2 and src.stride(1) == 1 and dst.stride(1) == 1
    _lib.check(lib.nm_copy_cols(_stream(), src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0),
                                src.shape[0], src.shape[1]), "nm_copy_cols")


def reduce_sum(x, out):
    lib = _lib.load()
    assert x.is_contiguous()
    _lib.check(lib.nm_reduce_sum(_stream(), x.data_ptr(), x.numel(), out.data_ptr()), "nm_reduce_sum")
    return out


def log_softmax_from_stats(x, rmax, rlse, out):
    lib = _lib.load()
    assert x.dim() == 2 and out.dim() == 2 and x.stride(1) == 1 and out.stride(1) == 1
    _lib.check(lib.nm_log_softmax(_stream(), x.data_ptr(), x.stride(0), rmax.data_ptr(), rlse.data_ptr(),
                                  out.data_ptr(), out.stride(0), x.shape[0], x.shape[1]), "nm_log_softmax")
    return out


def attn_workspace(rows, s, c, device):
    lib = _lib.load()
    nbytes = lib.nm_attn_workspace_bytes(rows, s, c)
    # zeroed ONCE: the tail holds the arrival counters of the in-kernel merge, which the kernels leave at zero
    return zero(torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device))


def gru_rh_seq(ru_all, hprev, out, lengths, ndir, hsz, reverse_dir0=False):
    lib = _lib.load()
    b, s = hprev.shape[0], hprev.shape[1]
    _lib.check(lib.nm_gru_rh_seq(_stream(), ru_all.data_ptr(), hprev.data_ptr(), out.data_ptr(),
                                 _p(lengths), _rev_mask(ndir, reverse_dir0), b, s, ndir, hsz),
               "nm_gru_rh_seq")


def attn_fwd(y, hf, states, mask, v, bias, rows_per_key, ctx, weights, workspace, energies_out=None):
    """Fused Bahdanau step.  y [R,A]; hf [Bk,S,A]; states [Bk,S,C]; mask [Bk,S]."""
    lib = _lib.load()
    r, a = y.shape
    _, s, c = states.shape
    assert hf.is_contiguous() and states.is_contiguous() and y.is_contiguous()
    assert ctx.stride(1) == 1
    _lib.check(lib.nm_attn_fwd(_stream(), y.data_ptr(), hf.data_ptr(), states.data_ptr(), _p(mask),
                               v.data_ptr(), _p(bias), r, rows_per_key, s, a, c, ctx.data_ptr(),
                               ctx.stride(0), _p(weights), workspace.data_ptr(),
                               workspace.numel() * 4, _p(energies_out)), "nm_attn_fwd")


def attn_fwd_time_major(y_all, hf, states, mask, v, bias, ctx_all, w_all, workspace, energies_out=None):
    """All T teacher-forced attention steps in one launch.  y_all [T,B,A] (time-major query
    projections), ctx_all [T,B,C], w_all / energies_out [T,B,S]; keys are read once per sentence."""
    lib = _lib.load()
    t, b, a = y_all.shape
    _, s, c = states.shape
    assert y_all.is_contiguous() and ctx_all.is_contiguous() and hf.is_contiguous() and states.is_contiguous()
    _lib.check(lib.nm_attn_fwd_multi(_stream(), y_all.data_ptr(), hf.data_ptr(), states.data_ptr(), _p(mask),
                                     v.data_ptr(), _p(bias), b, t, 1, b, s, a, c, ctx_all.data_ptr(), c,
                                     _p(w_all), workspace.data_ptr(), workspace.numel() * 4,
                                     _p(energies_out)), "nm_attn_fwd_multi")


def row_stats(x, rmax=None, lse=None, argmax=None):
    lib = _lib.load()
    assert x.dim() == 2 and x.stride(1) == 1
    _lib.check(lib.nm_row_stats(_stream(), x.data_ptr(), x.stride(0), x.shape[0], x.shape[1],
                                _p(rmax), _p(lse), _p(argmax)), "nm_row_stats")


def gumbel_argmax(x, salt: int, out):
    """One categorical draw per row from softmax(x) (tf.multinomial): argmax of x + Gumbel noise of (salt, row, col)."""
    lib = _lib.load()
    assert x.dim() == 2 and x.stride(1) == 1 and out.dtype == torch.int32
    _lib.check(lib.nm_gumbel_argmax(_stream(), x.data_ptr(), x.stride(0), x.shape[0], x.shape[1],
                                    int(salt) & 0xFFFFFFFF, out.data_ptr()), "nm_gumbel_argmax")


def greedy_update(argmax, finished, sym_out, mask_out, end_id, all_finished=None):
    lib = _lib.load()
    _lib.check(lib.nm_greedy_update(_stream(), argmax.data_ptr(), finished.data_ptr(),
                                    sym_out.data_ptr(), _p(mask_out), argmax.numel(), end_id,
                                    _p(all_finished)), "nm_greedy_update")


def xent(logits, targets, weights, loss_rows, grad_scale=None, write_grad=False, label_smoothing=0.0):
    lib = _lib.load()
    assert logits.dim() == 2 and logits.stride(1) == 1
    _lib.check(lib.nm_xent(_stream(), logits.data_ptr(), logits.stride(0), logits.shape[0],
                           logits.shape[1], targets.data_ptr(), _p(weights), _p(loss_rows),
                           _p(grad_scale), int(write_grad), float(label_smoothing)), "nm_xent")


XENT_COLSUM_ROWS = 256        # one 1024-thread workgroup per CU


def xent_colsum_ok(logits) -> bool:
    v = logits.shape[1]
    return (logits.is_cuda and v % 4 == 0 and v <= 32768 and logits.stride(0) % 4 == 0 and
            logits.data_ptr() % 16 == 0 and os.environ.get("NM_XENT_COLSUM", "1") != "0")


def xent_colsum(logits, targets, weights, loss_rows, grad_scale, label_smoothing, partial):
    """Cross entropy + in-place gradient as ``xent(..., write_grad=True)``; ``partial`` [G, V] receives per-workgroup
    column sums of the gradient (G <= rows): ``colsum(partial, bias_grad)`` is the projection's bias gradient."""
    lib = _lib.load()
    assert logits.dim() == 2 and logits.stride(1) == 1 and partial.is_contiguous()
    assert partial.shape[1] == logits.shape[1] and 1 <= partial.shape[0] <= logits.shape[0]
    _lib.check(lib.nm_xent_colsum(_stream(), logits.data_ptr(), logits.stride(0), logits.shape[0], logits.shape[1],
                                  targets.data_ptr(), _p(weights), _p(loss_rows), _p(grad_scale),
                                  float(label_smoothing), partial.data_ptr(), partial.shape[0]), "nm_xent_colsum")


def beam_workspace(b, k, v, device):
    lib = _lib.load()
    return torch.empty((lib.nm_beam_workspace_bytes(b, k, v) + 3) // 4, dtype=torch.float32, device=device)


def beam_topk_step(logits, b, k, rmax, rlse, logprob_sum, lengths, finished, penalty, end_id,
                   out_score, out_word, out_beam, out_logprob_sum, out_lengths, out_finished,
                   out_src_row, workspace, all_finished=None):
    lib = _lib.load()
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] == b * k
    _lib.check(lib.nm_beam_topk_step(_stream(), logits.data_ptr(), logits.stride(0), b, k,
                                     logits.shape[1], rmax.data_ptr(), rlse.data_ptr(),
                                     logprob_sum.data_ptr(), lengths.data_ptr(), finished.data_ptr(),
                                     penalty.data_ptr(), end_id, out_score.data_ptr(),
                                     out_word.data_ptr(), out_beam.data_ptr(),
                                     out_logprob_sum.data_ptr(), out_lengths.data_ptr(),
                                     out_finished.data_ptr(), out_src_row.data_ptr(),
                                     workspace.data_ptr(), workspace.numel() * 4, _p(all_finished)),
               "nm_beam_topk_step")


def beam_topk_step_fused(logits, b, k, logprob_sum, lengths, finished, penalty, end_id, out_score, out_word,
                         out_beam, out_logprob_sum, out_lengths, out_finished, out_src_row, workspace, rmax, rlse,
                         all_finished=None):
    """One beam body straight from the raw parent logits (row statistics fused into the scan)."""
    lib = _lib.load()
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] == b * k
    _lib.check(lib.nm_beam_topk_step_fused(
        _stream(), logits.data_ptr(), logits.stride(0), b, k, logits.shape[1], logprob_sum.data_ptr(),
        lengths.data_ptr(), finished.data_ptr(), penalty.data_ptr(), end_id, out_score.data_ptr(),
        out_word.data_ptr(), out_beam.data_ptr(), out_logprob_sum.data_ptr(), out_lengths.data_ptr(),
        out_finished.data_ptr(), out_src_row.data_ptr(), workspace.data_ptr(), workspace.numel() * 4,
        _p(all_finished), rmax.data_ptr(), rlse.data_ptr()), "nm_beam_topk_step_fused")


def logits_stats_numel(rows, vocab):
    """Floats of the per-tile row statistics ``logits_stats_gemm`` writes for [rows, vocab] logits."""
    return _lib.load().nm_logits_stats_bytes(rows, vocab) // 4


def logits_stats_buffer(rows, vocab, device):
    return torch.empty(logits_stats_numel(rows, vocab), dtype=torch.float32, device=device)


def logits_stats_gemm(state, w, bias, stats, out=None, trans_b=False):
    """logits = state . W + b with {max, sum exp, argmax} of every 128-column tile of every row written to
    ``stats``; the logits are stored only when ``out`` is given."""
    lib = _lib.load()
    _f32(state), _f32(w)
    m, k = state.shape
    n = w.shape[0] if trans_b else w.shape[1]
    assert state.stride(1) == 1 and w.stride(1) == 1 and (out is None or (out.stride(1) == 1 and out.shape == (m, n)))
    _lib.check(lib.nm_logits_stats_gemm(_stream(), int(trans_b), m, n, k, state.data_ptr(), state.stride(0),
                                        w.data_ptr(), w.stride(0), _p(bias), _p(out),
                                        out.stride(0) if out is not None else 0, stats.data_ptr(),
                                        stats.numel() * 4), "nm_logits_stats_gemm")


PROJ_SPLIT = os.environ.get("NM_PROJ_SPLIT", "0") == "1"


def proj_split_prepare(w, trans_b=False, planes=None):
    """OPT-IN (NM_PROJ_SPLIT=1): split the vocabulary projection's weights ``w`` ([K,N]; [N,K] with ``trans_b``) into
    three bf16 planes and register them: ``logits_stats_gemm`` with this ``w`` then runs six bf16 matrix-core products
    instead of the exact-fp32 kernel (nm_proj_split_prepare).  Returns the planes (keep them alive while ``w`` is
    registered; call again when ``w`` changes)."""
    lib = _lib.load()
    _f32(w)
    assert w.dim() == 2 and w.stride(1) == 1
    n, k = (w.shape[0], w.shape[1]) if trans_b else (w.shape[1], w.shape[0])
    nbytes = lib.nm_proj_split_bytes(n, k)
    if nbytes <= 0:
        return None
    if planes is None or planes.numel() * 2 < nbytes:
        planes = torch.empty(nbytes // 2, dtype=torch.int16, device=w.device)
    _lib.check(lib.nm_proj_split_prepare(_stream(), w.data_ptr(), w.stride(0), int(trans_b), n, k, planes.data_ptr(),
                                         planes.numel() * 2), "nm_proj_split_prepare")
    return planes


def proj_split_forget(w=None):
    _lib.check(_lib.load().nm_proj_split_forget(_p(w)), "nm_proj_split_forget")


def greedy_finish(stats, vocab, finished, sym_out, mask_out, end_id, all_finished=None, table=None, emb_out=None,
                  argmax_out=None, max_out=None, lse_out=None):
    """Greedy step tail from the tile statistics: argmax, symbol / finished update, next input embedding."""
    lib = _lib.load()
    rows = sym_out.numel()
    tile = lib.nm_logits_stats_tile(rows)
    ntiles = (vocab + tile - 1) // tile
    if emb_out is not None:
        assert emb_out.dim() == 2 and emb_out.stride(1) == 1 and emb_out.shape[0] == rows
    _lib.check(lib.nm_greedy_finish(_stream(), stats.data_ptr(), ntiles, rows, finished.data_ptr(),
                                    sym_out.data_ptr(), _p(mask_out), end_id, _p(all_finished), _p(table),
                                    table.shape[0] if table is not None else 0,
                                    table.shape[1] if table is not None else 0, _p(emb_out),
                                    emb_out.stride(0) if emb_out is not None else 0, _p(argmax_out), _p(max_out),
                                    _p(lse_out)), "nm_greedy_finish")


def beam_topk_step_tiles(logits, stats, b, k, logprob_sum, lengths, finished, penalty, end_id, out_score, out_word,
                         out_beam, out_logprob_sum, out_lengths, out_finished, out_src_row, workspace, rmax, rlse,
                         all_finished=None, tile=None):
    """One beam body from logits whose tile statistics ``logits_stats_gemm`` left in ``stats``.  ``tile`` (64 or
    128) names the width of statistics built elsewhere; by default it is the width ``logits_stats_gemm`` uses."""
    lib = _lib.load()
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] == b * k
    if tile is None:
        tile = lib.nm_logits_stats_tile(b * k)
    v = logits.shape[1]
    _lib.check(lib.nm_beam_topk_step_tiles(
        _stream(), logits.data_ptr(), logits.stride(0), stats.data_ptr(), tile, b, k, v,
        logprob_sum.data_ptr(), lengths.data_ptr(), finished.data_ptr(), penalty.data_ptr(), end_id,
        out_score.data_ptr(), out_word.data_ptr(), out_beam.data_ptr(), out_logprob_sum.data_ptr(),
        out_lengths.data_ptr(), out_finished.data_ptr(), out_src_row.data_ptr(), workspace.data_ptr(),
        workspace.numel() * 4, _p(all_finished), rmax.data_ptr(), rlse.data_ptr()), "nm_beam_topk_step_tiles")


def beam_topk_step_wide(logits, b, k, logprob_sum, lengths, finished, penalty, end_id, out_score, out_word, out_beam,
                        out_logprob_sum, out_lengths, out_finished, out_src_row, workspace, rmax=None, rlse=None,
                        all_finished=None, rmax_in=None, rlse_in=None, stats=None, tile=None):
    """One beam body for beams of up to 64 hypotheses.  Row statistics: ``rmax_in`` / ``rlse_in`` when given (the
    two-pass and ensemble convention), else the tile statistics ``stats`` of ``logits_stats_gemm``, else computed;
    in the last two cases they are left in ``rmax`` / ``rlse``."""
    lib = _lib.load()
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] == b * k
    if stats is not None and tile is None:
        tile = lib.nm_logits_stats_tile(b * k)
    _lib.check(lib.nm_beam_topk_step_wide(
        _stream(), logits.data_ptr(), logits.stride(0), b, k, logits.shape[1], logprob_sum.data_ptr(),
        lengths.data_ptr(), finished.data_ptr(), penalty.data_ptr(), end_id, _p(out_score), _p(out_word),
        _p(out_beam), _p(out_logprob_sum), _p(out_lengths), _p(out_finished), _p(out_src_row), _p(workspace),
        0 if workspace is None else workspace.numel() * workspace.element_size(), _p(all_finished), _p(rmax), _p(rlse),
        _p(rmax_in), _p(rlse_in), _p(stats), tile or 0), "nm_beam_topk_step_wide")


def sample_step(logits, salt_base, salt_step: int, end_id: int, finished, logprob_sum, lengths, out_symbol, out_logprob,
                out_kept, out_finished, out_logprob_sum, out_lengths, temperature: float = 1.0, top_k: int = 0,
                top_p: float = 1.0, all_finished=None, workspace=None, inv_temperature: Optional[float] = None):
    """One truncated sampling step per row of ``logits`` (nm_sample_step, include/nmhip_sample.h): temperature, top-k,
    then nucleus truncation; the draw is nm_gumbel_argmax's over the kept entries with the salt
    ``salt_base[0] + salt_step`` (``salt_base``: one int32 / uint32 word on the device, so that a captured graph
    draws afresh when the word is rewritten); per row the symbol, its log-probability under the truncated
    distribution, the size of the kept set, and the loop state (finished, summed log-probability, length).  The
    kernel multiplies by ``inv_temperature`` (default: 1 / temperature rounded to float32)."""
    lib = _lib.load()
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.dtype == torch.float32
    assert salt_base.numel() == 1 and salt_base.element_size() == 4
    inv_t = float(inv_temperature) if inv_temperature is not None else 1.0 / float(temperature)
    _lib.check(lib.nm_sample_step(
        _stream(), logits.data_ptr(), logits.stride(0), logits.shape[0], logits.shape[1], inv_t, int(top_k),
        float(top_p), salt_base.data_ptr(), int(salt_step) & 0xFFFFFFFF, end_id, finished.data_ptr(),
        logprob_sum.data_ptr(), lengths.data_ptr(), out_symbol.data_ptr(), out_logprob.data_ptr(), out_kept.data_ptr(),
        out_finished.data_ptr(), out_logprob_sum.data_ptr(), out_lengths.data_ptr(), _p(all_finished), _p(workspace),
        0 if workspace is None else workspace.numel() * workspace.element_size()), "nm_sample_step")


def attn_partials_layout(rows, s, a, c):
    """(nchunk, pctx offset, pstat offset) in floats inside the attention workspace, or None when the shape is
    served by the any-shape kernel (no split-S partials)."""
    lib = _lib.load()
    n, po, so = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    if lib.nm_attn_partials_layout(rows, s, a, c, ctypes.byref(n), ctypes.byref(po), ctypes.byref(so)) != 0:
        return None
    return int(n.value), int(po.value), int(so.value)


def attn_fwd_partials(y, hf, states, mask, v, bias, rows_per_key, workspace):
    """The attention step without its combine launch: energies + split-S partials stay in ``workspace``."""
    lib = _lib.load()
    r, a = y.shape
    _, s, c = states.shape
    assert hf.is_contiguous() and states.is_contiguous() and y.is_contiguous()
    _lib.check(lib.nm_attn_fwd_partials(_stream(), y.data_ptr(), hf.data_ptr(), states.data_ptr(), _p(mask),
                                        v.data_ptr(), _p(bias), r, rows_per_key, s, a, c, workspace.data_ptr(),
                                        workspace.numel() * 4), "nm_attn_fwd_partials")


class StepGroup:
    """A launch of ``nm_step_group``: problem descriptors are built once (all pointers are persistent buffers)
    and re-launched every step; ``patch`` changes the per-step pointers (history rows)."""

    def __init__(self, rows, problems):
        lib = _lib.load()
        self.rows = rows
        self.keep = []                       # tensors the descriptors point into
        self.arr = (_lib.StepProblem * len(problems))()
        for slot, spec in zip(self.arr, problems):
            for name, val in spec.items():
                if isinstance(val, torch.Tensor):
                    self.keep.append(val)
                    val = val.data_ptr()
                setattr(slot, name, val)
        self._fn = lib.nm_step_group

    def patch(self, index, **fields):
        for name, val in fields.items():
            setattr(self.arr[index], name, val.data_ptr() if isinstance(val, torch.Tensor) else (val or 0))

    def launch(self):
        _lib.check(self._fn(_stream(), self.rows, self.arr, len(self.arr)), "nm_step_group")

    def plan(self):
        """The kernel ``launch`` would run (a name of ``STEP_GROUP_PLANS``), chosen by the library's own rule;
        descriptors ``launch`` would refuse raise the same error.  Nothing is launched."""
        code = _lib.load().nm_step_group_plan(self.rows, self.arr, len(self.arr))
        if code < 0:
            _lib.check(code, "nm_step_group_plan")
        return STEP_GROUP_PLANS[code]


# the NM_STEP_PLAN_* codes of include/nmhip.h, in order
STEP_GROUP_PLANS = ("16x1", "16x2", "16x1-partials", "medium-4x2x2", "medium-8x1x1", "medium-4x1x1", "dma")


class DecoderStepCall:
    """``nm_decoder_step_fused``: the descriptor of a whole decoder step, built once from persistent buffers;
    ``launch`` patches the per-step pointers (history rows, outputs) and makes the one call."""

    def __init__(self, fields):
        lib = _lib.load()
        self.keep = {}
        self.desc = _lib.DecoderStep()
        self._set(fields)
        self._fn = lib.nm_decoder_step_fused

    def _set(self, fields):
        for name, val in fields.items():
            if isinstance(val, torch.Tensor):
                self.keep[name] = val
                val = val.data_ptr()
            setattr(self.desc, name, val or 0)

    def launch(self, **fields):
        self._set(fields)
        _lib.check(self._fn(_stream(), ctypes.byref(self.desc)), "nm_decoder_step_fused")


def gather_rows(src, idx, dst):
    lib = _lib.load()
    assert src.dim() == 2 and dst.dim() == 2 and src.stride(1) == 1 and dst.stride(1) == 1
    _lib.check(lib.nm_gather_rows_f32(_stream(), src.data_ptr(), src.stride(0), idx.data_ptr(),
                                      dst.data_ptr(), dst.stride(0), dst.shape[0], dst.shape[1]),
               "nm_gather_rows_f32")


def beam_reorder_tokens(src, src_row, word, dst, steps, rows):
    lib = _lib.load()
    _lib.check(lib.nm_beam_reorder_tokens(_stream(), src.data_ptr(), src_row.data_ptr(),
                                          word.data_ptr(), dst.data_ptr(), steps, rows),
               "nm_beam_reorder_tokens")


def beam_backtrace(src_hist, word_hist, first, out, steps):
    """Token histories [steps+1, R] from the per-step (source row, word) records of a beam search."""
    lib = _lib.load()
    rows = first.numel()
    assert src_hist.is_contiguous() and word_hist.is_contiguous() and out.is_contiguous()
    assert src_hist.shape[1] == rows and word_hist.shape[1] == rows and out.shape[1] == rows and out.shape[0] > steps
    _lib.check(lib.nm_beam_backtrace(_stream(), src_hist.data_ptr(), word_hist.data_ptr(), first.data_ptr(),
                                     out.data_ptr(), steps, rows), "nm_beam_backtrace")


def length_penalty_table(max_len: int, alpha: float, device) -> torch.Tensor:
    """((5+len)/6)**alpha for len in [0, max_len], evaluated in fp32 on the host
    the way the reference's tf.pow sees it (beam_search_decoder.py:561-573)."""
    lens = np.arange(max_len + 1, dtype=np.float32)
    tab = ((np.float32(5.0) + lens) / np.float32(6.0)) ** np.float32(alpha)
    return torch.from_numpy(tab.astype(np.float32)).to(device)


# ---- backward / trainer kernels ------------------------------------------------
def tanh_bwd(dy, y):
    lib = _lib.load()
    assert dy.is_contiguous() and y.is_contiguous() and dy.numel() == y.numel()
    _lib.check(lib.nm_tanh_bwd(_stream(), dy.data_ptr(), y.data_ptr(), dy.numel()), "nm_tanh_bwd")
    return dy


_COLSUM_WS = {}


def _colsum_workspace(device, cols):
    key = (device, cols, _stream(), workspace_tag())
    ws = _COLSUM_WS.get(key)
    if ws is None:
        # zeroed ONCE: the tail holds the arrival counters of the in-kernel final pass, which the kernel leaves at zero
        # (created inside a stream capture when the capture stream is new to this cache: the fill below is then a node
        # of that graph, replayed with it -- the library's fill, not a tensor library's)
        ws = zero(torch.empty(_lib.load().nm_colsum_workspace_bytes(cols) // 4, dtype=torch.float32, device=device))
        _COLSUM_WS[key] = ws
    return ws


def colsum(x, out, accumulate=False):
    """out[c] (+)= sum_r x[r,c] (bias gradients); deterministic."""
    lib = _lib.load()
    assert x.dim() == 2 and x.stride(1) == 1
    cols = x.shape[1]
    ws = _colsum_workspace(x.device, cols)
    # (on a side stream -- runtime.Session.side -- the launch runs beside a time loop: the low-pressure kernel)
    _lib.check(lib.nm_colsum_algo(_stream(), x.data_ptr(), x.stride(0), x.shape[0], cols, out.data_ptr(),
                                  int(accumulate), ws.data_ptr(), ws.numel() * 4,
                                  1 if getattr(_TLS, "on_side", False) else 0), "nm_colsum")
    return out


def embedding_scatter_add(dtable, ids, d, skip_pad=False):
    lib = _lib.load()
    assert d.dim() == 2 and d.stride(1) == 1 and dtable.is_contiguous()
    _lib.check(lib.nm_embedding_scatter_add(_stream(), dtable.data_ptr(), dtable.shape[0], dtable.shape[1],
                                            ids.data_ptr(), ids.numel(), d.data_ptr(), d.stride(0),
                                            int(skip_pad)), "nm_embedding_scatter_add")


_LNB_WS = {}


def _layer_norm_bwd_workspace(device, d):
    """The [G][2][D] partial sums between nm_layer_norm_bwd_params' main kernel and its reduce launch, one buffer per
    (device, width, stream, tag) like the column sums': two launches of one width on two streams must not share it."""
    key = (device, d, _stream(), workspace_tag())
    ws = _LNB_WS.get(key)
    if ws is None:
        ws = _LNB_WS[key] = torch.empty(_lib.load().nm_layer_norm_bwd_params_workspace_bytes(d) // 4,
                                        dtype=torch.float32, device=device)
    return ws


def layer_norm_bwd_params(dy, x, mean, rstd, gamma, dx, dgamma, dbeta, accumulate=True, accumulate_dx=False):
    """dx of a layer norm and its parameter gradients in one call (nm_layer_norm_bwd_params); ``accumulate_dx``: dx is
    added to what ``dx`` holds."""
    lib = _lib.load()
    d = x.shape[-1]
    rows = x.numel() // d
    assert dy.is_contiguous() and x.is_contiguous() and dx.is_contiguous()
    ws = _layer_norm_bwd_workspace(x.device, d)
    _lib.check(lib.nm_layer_norm_bwd_params(_stream(), dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                            gamma.data_ptr(), dx.data_ptr(), rows, d, dgamma.data_ptr(),
                                            dbeta.data_ptr(), int(bool(accumulate)) | (2 if accumulate_dx else 0),
                                            ws.data_ptr(), ws.numel() * 4), "nm_layer_norm_bwd_params")


def layer_norm_bwd(dy, x, mean, rstd, gamma, dx, dyx):
    lib = _lib.load()
    d = x.shape[-1]
    rows = x.numel() // d
    assert dy.is_contiguous() and x.is_contiguous() and dx.is_contiguous() and dyx.is_contiguous()
    _lib.check(lib.nm_layer_norm_bwd(_stream(), dy.data_ptr(), x.data_ptr(), mean.data_ptr(),
                                     rstd.data_ptr(), gamma.data_ptr(), dx.data_ptr(), dyx.data_ptr(),
                                     rows, d), "nm_layer_norm_bwd")


def gru_step_bwd(phase, dh, dout, dout_strides, ru, c, h0, hseq, hseq_strides, dxp, dxp_strides, dgpre,
                 dcpre, drh, lengths, t, ndir, rows, hsz, reverse_dir0=False):
    """phase 0 = blend backward, phase 1 = gates backward (nm_backward.hip)."""
    lib = _lib.load()
    do = dout_strides or (0, 0, 0)
    _lib.check(lib.nm_gru_step_bwd(_stream(), phase, dh.data_ptr(), _p(dout), do[0], do[1], do[2],
                                   ru.data_ptr(), _p(c), _p(h0), hseq.data_ptr(), hseq_strides[0],
                                   hseq_strides[1], hseq_strides[2], dxp.data_ptr(), dxp_strides[0],
                                   dxp_strides[1], dxp_strides[2], dgpre.data_ptr(), _p(dcpre), _p(drh),
                                   _p(lengths), t, _rev_mask(ndir, reverse_dir0), ndir, rows, hsz),
               "nm_gru_step_bwd")


def gru_seq_shift(seq, out, lengths, ndir, hsz, reverse_dir0=False):
    lib = _lib.load()
    b, s = seq.shape[0], seq.shape[1]
    _lib.check(lib.nm_gru_seq_shift(_stream(), seq.data_ptr(), out.data_ptr(), _p(lengths),
                                    _rev_mask(ndir, reverse_dir0), b, s, ndir, hsz), "nm_gru_seq_shift")


def attn_softmax_bwd(dw, e, mask, de, bsz):
    lib = _lib.load()
    s = dw.shape[-1]
    rows = dw.numel() // s
    _lib.check(lib.nm_attn_softmax_bwd(_stream(), dw.data_ptr(), e.data_ptr(), _p(mask), de.data_ptr(),
                                       rows, bsz, s), "nm_attn_softmax_bwd")


def attn_step_bwd(dctx, states, e, mask, hf, y, v, de, dy):
    """One step's attention backward up to the query in one launch: dctx [B,C] (rows may be strided), states [B,S,C],
    e [B,S] the step's energies, hf [B,S,A], y [B,A] -> de [B,S] (written), dy [B,A] (written)."""
    lib = _lib.load()
    b, s, c = states.shape
    a = hf.shape[2]
    assert states.is_contiguous() and hf.is_contiguous() and e.is_contiguous() and de.is_contiguous()
    assert dctx.stride(1) == 1 and y.stride(1) == 1 and dy.stride(1) == 1
    _lib.check(lib.nm_attn_step_bwd(_stream(), dctx.data_ptr(), dctx.stride(0), states.data_ptr(), e.data_ptr(), _p(mask),
                                    hf.data_ptr(), y.data_ptr(), y.stride(0), v.data_ptr(), de.data_ptr(), dy.data_ptr(),
                                    dy.stride(0), b, s, c, a), "nm_attn_step_bwd")


def attn_step_bwd_ok(dctx, c) -> bool:
    return dctx.is_cuda and c % 4 == 0 and dctx.stride(0) % 4 == 0 and dctx.data_ptr() % 16 == 0


def attn_softmax_fwd(e, mask, w, bsz, rows_per_key=1):
    """w = renorm(softmax(e) * mask) of contiguous [R,S] energies assembled by the caller."""
    lib = _lib.load()
    assert e.is_contiguous() and w.is_contiguous() and e.shape == w.shape
    s = e.shape[-1]
    rows = e.numel() // s
    _lib.check(lib.nm_attn_softmax_fwd(_stream(), e.data_ptr(), _p(mask), w.data_ptr(), rows, bsz, s,
                                       rows_per_key), "nm_attn_softmax_fwd")
    return w


def attn_energy_bwd(de, hf, y, v, dhf, dv_partial, dy, accumulate=False):
    """Energies backward of T queries per sentence (nm_attn_energy_bwd); ``dhf`` and ``dv_partial`` both None: the query
    gradients ``dy`` alone."""
    lib = _lib.load()
    t, b, s = de.shape
    a = hf.shape[-1]
    assert de.is_contiguous() and y.is_contiguous() and dy.is_contiguous()
    _lib.check(lib.nm_attn_energy_bwd(_stream(), de.data_ptr(), hf.data_ptr(), y.data_ptr(), v.data_ptr(),
                                      _p(dhf), _p(dv_partial), dy.data_ptr(), t, b, s, a,
                                      int(accumulate)), "nm_attn_energy_bwd")


# ---- strided element-wise primitives (general / taped path) -------------------------------------
EW = {"copy": 0, "add": 1, "sub": 2, "mul": 3, "scale": 4, "sigmoid": 5, "tanh": 6, "relu": 7,
      "sigmoid_bwd": 8, "tanh_bwd": 9, "relu_bwd": 10, "logaddexp": 11, "add_scalar": 12, "rowscale": 13, "div": 14}


def _rc(t):
    """(rows, cols, ld) of a 1-D / 2-D / contiguous n-D float tensor with unit inner stride."""
    _f32(t)
    if t.dim() == 2:
        assert t.stride(1) == 1 or t.shape[1] == 1
        return t.shape[0], t.shape[1], t.stride(0)
    assert t.is_contiguous(), "n-D operands of element-wise kernels must be contiguous"
    return 1, t.numel(), t.numel()


def zero_if(word, x):
    """``x[:] = 0`` when the int32 device word is not zero (nm_zero_if): the gradient of a step whose time loop gave up
    must not reach an accumulation buffer or a collective as NaNs."""
    _lib.check(_lib.load().nm_zero_if(_stream(), word.data_ptr(), x.data_ptr(), x.numel()), "nm_zero_if")


def fill(x, value=0):
    """``x[:] = value`` for a contiguous float32 / int32 buffer with the library's fill kernel (nm_fill_u32).  Other
    tensors (host tensors, other dtypes, strided views) take torch's fill."""
    if not x.is_cuda or not x.is_contiguous() or x.dtype not in (torch.float32, torch.int32):
        return x.fill_(value)
    if x.dtype == torch.float32:
        pattern = struct.unpack("<I", struct.pack("<f", float(value)))[0]
    else:
        pattern = int(value) & 0xFFFFFFFF
    _lib.check(_lib.load().nm_fill_u32(_stream(), x.data_ptr(), x.numel(), pattern), "nm_fill_u32")
    return x


def zero(x):
    return fill(x, 0)


def copy(dst, src):
    """``dst[:] = src`` for two contiguous device buffers of one dtype and size as a runtime device-to-device copy
    (nm_copy_d2d: a memcpy node inside a captured graph); anything else takes torch's copy_."""
    if (dst.is_cuda and src.is_cuda and dst.dtype == src.dtype and dst.numel() == src.numel() and dst.is_contiguous()
            and src.is_contiguous() and dst.device == src.device):
        _lib.check(_lib.load().nm_copy_d2d(_stream(), dst.data_ptr(), src.data_ptr(), dst.numel() * dst.element_size()),
                   "nm_copy_d2d")
        return dst
    return dst.copy_(src)


def ew(op, a, b, out, alpha=0.0, accumulate=False):
    """out (+)= op(a, b) element-wise; 2-D operands may be column slices (row stride = ld)."""
    lib = _lib.load()
    rows, cols, lda = _rc(a)
    ro, co, ldo = _rc(out)
    assert (rows, cols) == (ro, co), (a.shape, out.shape)
    ldb = 0
    if b is not None:
        rb, cb, ldb = _rc(b)
        assert (rb, cb) == ((rows, 1) if op == "rowscale" else (rows, cols)), (a.shape, b.shape)
    _lib.check(lib.nm_ew(_stream(), EW[op], a.data_ptr(), lda, _p(b), ldb, out.data_ptr(), ldo, rows, cols,
                         float(alpha), int(accumulate)), "nm_ew")
    return out


def blend_fwd(u, h, c, out):
    lib = _lib.load()
    rows, cols, ldu = _rc(u)
    _lib.check(lib.nm_blend_fwd(_stream(), u.data_ptr(), ldu, h.data_ptr(), _rc(h)[2], c.data_ptr(), _rc(c)[2],
                                out.data_ptr(), _rc(out)[2], rows, cols), "nm_blend_fwd")
    return out


def lstm_cell_fwd(z, c_prev, c_new, h_new, gates=None, forget_bias=1.0):
    """One LSTMCell step after its products: z [R,4H] (i, j, f, o) -> c', h' (+ the activated gates)."""
    lib = _lib.load()
    rows, h = c_prev.shape
    assert z.shape == (rows, 4 * h) and z.stride(1) == 1
    _lib.check(lib.nm_lstm_cell_fwd(_stream(), z.data_ptr(), z.stride(0), c_prev.data_ptr(), _rc(c_prev)[2],
                                    c_new.data_ptr(), _rc(c_new)[2], h_new.data_ptr(), _rc(h_new)[2], _p(gates),
                                    0 if gates is None else gates.stride(0), rows, h, float(forget_bias)),
               "nm_lstm_cell_fwd")


def lstm_cell_bwd(dh, dc_new, gates, c_prev, c_new, dz, dc_prev, accumulate_dz=False, accumulate_dc_prev=False):
    lib = _lib.load()
    rows, h = c_prev.shape
    ld = lambda t: 0 if t is None else _rc(t)[2]
    _lib.check(lib.nm_lstm_cell_bwd(_stream(), _p(dh), ld(dh), _p(dc_new), ld(dc_new), gates.data_ptr(),
                                    gates.stride(0), c_prev.data_ptr(), ld(c_prev), c_new.data_ptr(), ld(c_new),
                                    dz.data_ptr(), dz.stride(0), _p(dc_prev), ld(dc_prev), rows, h,
                                    int(accumulate_dz), int(accumulate_dc_prev)), "nm_lstm_cell_bwd")


def nematus_state_step_ok(h_prev, w_st, h_new) -> bool:
    """The one-launch step takes it, and pays: up to 512 tiles of 16 rows x 16 units (two per compute unit).  Beyond
    that -- 640 beam rows x 512 units are 1280 -- the product on large tiles and the point-wise launch are faster
    (beam-5 of the general path 24.6 against 25.0 ms per batch)."""
    rows, h = h_prev.shape
    if ((rows + 15) // 16) * ((h + 15) // 16) > 512 or h % 8:
        return False
    return (h_prev.is_cuda and h_prev.stride(1) == 1 and h_prev.stride(0) % 4 == 0 and h_prev.data_ptr() % 16 == 0
            and w_st.stride(1) == 1 and h_new.stride(1) == 1 and h_new.data_ptr() != h_prev.data_ptr())


def nematus_state_step(h_prev, w_st, b_st, x_all, h_new, ru=None, c_out=None, sc_out=None):
    """h_new = NematusGRUCell step from the previous state [R,H], the state kernels [H,3H] = [U_g | U_c] (+ bias [3H]) and
    the projected input half x_all [R,3H]: product and point-wise part in ONE launch (nm_nematus_state_step).  ru [R,2H],
    c_out [R,H] (contiguous) and sc_out [R,H] (row stride free) keep what the backward pass reads."""
    lib = _lib.load()
    rows, h = h_prev.shape
    assert w_st.shape == (h, 3 * h) and x_all.shape == (rows, 3 * h) and h_new.shape == (rows, h) and x_all.stride(1) == 1
    assert ru is None or ru.is_contiguous()
    assert c_out is None or c_out.is_contiguous()
    assert sc_out is None or sc_out.stride(1) == 1
    _lib.check(lib.nm_nematus_state_step(_stream(), h_prev.data_ptr(), h_prev.stride(0), w_st.data_ptr(), w_st.stride(0),
                                         _p(b_st), x_all.data_ptr(), x_all.stride(0), h_new.data_ptr(), h_new.stride(0),
                                         _p(ru), _p(c_out), _p(sc_out), 0 if sc_out is None else sc_out.stride(0), rows, h),
               "nm_nematus_state_step")


def nematus_full_step_ok(x, w_in) -> bool:
    """(beside nematus_state_step_ok) the step's input rows can be multiplied in the same launch"""
    d = x.shape[1]
    return (d % 8 == 0 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and w_in.stride(1) == 1)


def nematus_full_step(h_prev, w_st, b_st, x, w_in, b_in, h_new, ru=None, c_out=None, sc_out=None):
    """nematus_state_step with the input half x [R,D] . w_in [D,3H] (+ b_in) computed in the same launch."""
    lib = _lib.load()
    rows, h = h_prev.shape
    d = x.shape[1]
    assert w_st.shape == (h, 3 * h) and w_in.shape == (d, 3 * h) and x.shape[0] == rows and h_new.shape == (rows, h)
    assert ru is None or ru.is_contiguous()
    assert c_out is None or c_out.is_contiguous()
    assert sc_out is None or sc_out.stride(1) == 1
    _lib.check(lib.nm_nematus_full_step(_stream(), h_prev.data_ptr(), h_prev.stride(0), w_st.data_ptr(), w_st.stride(0),
                                        _p(b_st), x.data_ptr(), x.stride(0), w_in.data_ptr(), w_in.stride(0), _p(b_in),
                                        h_new.data_ptr(), h_new.stride(0), _p(ru), _p(c_out), _p(sc_out),
                                        0 if sc_out is None else sc_out.stride(0), rows, h, d), "nm_nematus_full_step")


def nematus_cell_fwd(g_pre, sc, ci, h_prev, h_new, ru=None, c_out=None, g2=None):
    """h' of one NematusGRUCell step from its products (nm_nematus_cell_fwd); ``ru`` [R,2H] / ``c_out`` [R,H]: contiguous
    buffers for the backward call; ``g2``: a second gate operand added to ``g_pre``."""
    rows, h = h_prev.shape
    assert g_pre.shape == (rows, 2 * h) and (ru is None or ru.is_contiguous()) and (c_out is None or c_out.is_contiguous())
    _lib.check(_lib.load().nm_nematus_cell_fwd(_stream(), g_pre.data_ptr(), _rc(g_pre)[2], sc.data_ptr(), _rc(sc)[2],
                                               ci.data_ptr(), _rc(ci)[2], h_prev.data_ptr(), _rc(h_prev)[2],
                                               h_new.data_ptr(), _rc(h_new)[2], _p(ru), _p(c_out), _p(g2),
                                               0 if g2 is None else _rc(g2)[2], rows, h), "nm_nematus_cell_fwd")
    return h_new


def nematus_cell_bwd(dh, ru, c, sc, h_prev, dg, dci, dsc, dh_prev, acc_dg=False, acc_dci=False, acc_dsc=False,
                     acc_dh_prev=False, dg2=None):
    rows, h = h_prev.shape
    ld = lambda t: 0 if t is None else _rc(t)[2]
    _lib.check(_lib.load().nm_nematus_cell_bwd(_stream(), dh.data_ptr(), ld(dh), ru.data_ptr(), c.data_ptr(), sc.data_ptr(),
                                               ld(sc), h_prev.data_ptr(), ld(h_prev), dg.data_ptr(), ld(dg), _p(dci), ld(dci),
                                               _p(dsc), ld(dsc), _p(dh_prev), ld(dh_prev), _p(dg2), ld(dg2), rows, h, int(acc_dg),
                                               int(acc_dci), int(acc_dsc), int(acc_dh_prev)), "nm_nematus_cell_bwd")


def blend_bwd(dy, u, h, c, du, dh, dc):
    lib = _lib.load()
    rows, cols, ldu = _rc(u)
    ld = lambda t: 0 if t is None else _rc(t)[2]
    _lib.check(lib.nm_blend_bwd(_stream(), dy.data_ptr(), _rc(dy)[2], u.data_ptr(), ldu, h.data_ptr(), ld(h),
                                c.data_ptr(), ld(c), _p(du), ld(du), _p(dh), ld(dh), _p(dc), ld(dc), rows, cols),
               "nm_blend_bwd")


def dropout_salt(*parts) -> int:
    """32-bit salt of a dropout call site: crc32 of the "/"-joined parts (restated by the CPU checker in tests)."""
    import zlib
    return zlib.crc32("/".join(str(p) for p in parts).encode()) & 0xFFFFFFFF


def dropout(x, out, keep_prob, salt, accumulate=False, step=None):
    """``step``: optional int32 device scalar (global step) that advances the salt on the device."""
    lib = _lib.load()
    rows, cols, ldx = _rc(x)
    _lib.check(lib.nm_dropout(_stream(), x.data_ptr(), ldx, out.data_ptr(), _rc(out)[2], rows, cols,
                              float(keep_prob), int(salt) & 0xFFFFFFFF, _p(step), int(accumulate)), "nm_dropout")
    return out


def rnn_select_fwd(h_new, h_prev, lengths, t, h_out, y_out):
    lib = _lib.load()
    rows, cols, ldn = _rc(h_new)
    _lib.check(lib.nm_rnn_select_fwd(_stream(), h_new.data_ptr(), ldn, h_prev.data_ptr(), _rc(h_prev)[2],
                                     _p(lengths), t, h_out.data_ptr(), _rc(h_out)[2], _p(y_out),
                                     0 if y_out is None else _rc(y_out)[2], rows, cols), "nm_rnn_select_fwd")


def rnn_select_bwd(dh, dy, lengths, t, d_new, d_prev):
    lib = _lib.load()
    rows, cols, ldn = _rc(d_new)
    ld = lambda x: 0 if x is None else _rc(x)[2]
    _lib.check(lib.nm_rnn_select_bwd(_stream(), _p(dh), ld(dh), _p(dy), ld(dy), _p(lengths), t, d_new.data_ptr(),
                                     ldn, _p(d_prev), ld(d_prev), rows, cols), "nm_rnn_select_bwd")


def reverse_sequence(x, out, lengths, accumulate=False):
    lib = _lib.load()
    b, s, d = x.shape
    assert x.is_contiguous() and out.is_contiguous() and out.shape == x.shape
    _lib.check(lib.nm_reverse_sequence(_stream(), x.data_ptr(), out.data_ptr(), _i32(lengths).data_ptr(), b, s, d,
                                       int(accumulate)), "nm_reverse_sequence")
    return out


def maxout_fwd(x, out, argmax, pool=2):
    lib = _lib.load()
    rows, cols, ldx = _rc(x)
    groups = cols // pool
    assert groups * pool == cols and out.shape[1] == groups
    _lib.check(lib.nm_maxout_fwd(_stream(), x.data_ptr(), ldx, out.data_ptr(), _rc(out)[2], _p(argmax), rows,
                                 groups, pool), "nm_maxout_fwd")
    return out


def _bs(t):
    """Batch stride (floats) of a [B, T, D] tensor whose rows are contiguous."""
    assert t.dim() == 3 and t.stride(2) == 1 and t.stride(1) == t.shape[2], (t.shape, t.stride())
    return t.stride(0)


def sdp_attn_fwd(q, k, v, key_mask, heads, ctx, weights=None, causal=False, rows_per_key=1, keep_prob=1.0,
                 salt=0, step=None):
    """Multi-head scaled dot-product attention.  q/ctx [Bq,Tq,D], k/v [Bk,Tk,D] (Bq = Bk*rows_per_key;
    batch strides may exceed T*D: a key/value cache), key_mask [Bk,Tk] or None, weights [Bq,H,Tq,Tk]."""
    lib = _lib.load()
    bq, tq, d = q.shape
    bk, tk, _ = k.shape
    assert d % heads == 0 and bq == bk * rows_per_key and v.shape[1] == tk
    mask_bs = 0
    if key_mask is not None:
        assert key_mask.dim() == 2 and key_mask.stride(1) == 1 and key_mask.shape[1] >= tk
        mask_bs = key_mask.stride(0)
    if weights is not None:
        assert weights.is_contiguous() and weights.numel() == bq * heads * tq * tk
    _lib.check(lib.nm_sdp_attn_fwd(_stream(), q.data_ptr(), _bs(q), k.data_ptr(), _bs(k), v.data_ptr(), _bs(v),
                                   _p(key_mask), mask_bs, bq, rows_per_key, tq, tk, heads, d // heads, int(causal),
                                   float(keep_prob), int(salt) & 0xFFFFFFFF, _p(step), ctx.data_ptr(), _bs(ctx),
                                   _p(weights)), "nm_sdp_attn_fwd")
    return ctx


def sdp_attn_step(q, k, v, key_mask, heads, ancestors, ctx, weights=None):
    """One cached decoding step: q/ctx [R,1,D]; k/v [R,Tk,D] views of the caches; position j of row r is read from
    cache row ``ancestors[r, j]`` (int32 [R, >=Tk])."""
    lib = _lib.load()
    rows, tq, d = q.shape
    tk = k.shape[1]
    assert tq == 1 and d % heads == 0 and ancestors.dtype == torch.int32 and ancestors.stride(1) == 1
    assert ancestors.shape[0] == rows and ancestors.shape[1] >= tk
    mask_bs = 0
    if key_mask is not None:
        assert key_mask.dim() == 2 and key_mask.stride(1) == 1 and key_mask.shape[1] >= tk
        mask_bs = key_mask.stride(0)
    _lib.check(lib.nm_sdp_attn_step(_stream(), q.data_ptr(), _bs(q), k.data_ptr(), _bs(k), v.data_ptr(), _bs(v),
                                    _p(key_mask), mask_bs, rows, tk, heads, d // heads, ancestors.data_ptr(),
                                    ancestors.stride(0), ctx.data_ptr(), _bs(ctx), _p(weights)), "nm_sdp_attn_step")
    return ctx


def sdp_attn_bwd(q, k, v, key_mask, weights, dctx, heads, dq, dk, dv, de_ws, causal=False, keep_prob=1.0, salt=0,
                 accumulate=False, step=None):
    lib = _lib.load()
    b, tq, d = q.shape
    tk = k.shape[1]
    mask_bs = 0 if key_mask is None else key_mask.stride(0)
    assert de_ws.numel() >= b * heads * tq * tk
    _lib.check(lib.nm_sdp_attn_bwd(_stream(), q.data_ptr(), _bs(q), k.data_ptr(), _bs(k), v.data_ptr(), _bs(v),
                                   _p(key_mask), mask_bs, weights.data_ptr(), dctx.data_ptr(), _bs(dctx), b, tq, tk,
                                   heads, d // heads, int(causal), float(keep_prob), int(salt) & 0xFFFFFFFF,
                                   _p(step), dq.data_ptr(), _bs(dq), dk.data_ptr(), _bs(dk), dv.data_ptr(), _bs(dv),
                                   de_ws.data_ptr(), int(accumulate)), "nm_sdp_attn_bwd")


def add_position(x, signal, out, t0=0):
    """out[b,t,:] = x[b,t,:] + signal[t0+t,:]; x [B,T,D] contiguous, signal [Tmax,D]."""
    lib = _lib.load()
    b, t, d = x.shape
    assert x.is_contiguous() and out.is_contiguous() and signal.is_contiguous()
    assert signal.shape[1] == d and signal.shape[0] >= t0 + t
    _lib.check(lib.nm_add_position(_stream(), x.data_ptr(), signal.data_ptr(), out.data_ptr(), b, t, d, t0),
               "nm_add_position")
    return out


def unfinished_mask(finished, out_col):
    """out_col[r] = 0.0 where finished[r] else 1.0; ``out_col`` may be a strided column view."""
    lib = _lib.load()
    n = finished.numel()
    assert out_col.dim() == 1 and out_col.numel() == n
    _lib.check(lib.nm_unfinished_mask(_stream(), _i32(finished).data_ptr(), out_col.data_ptr(),
                                      out_col.stride(0) if n > 1 else 1, n), "nm_unfinished_mask")


def time_sum(x, out):
    lib = _lib.load()
    b, t, d = x.shape
    assert x.is_contiguous() and out.is_contiguous()
    _lib.check(lib.nm_time_sum(_stream(), x.data_ptr(), out.data_ptr(), b, t, d), "nm_time_sum")
    return out


def time_bcast_add(dy, dx):
    lib = _lib.load()
    b, t, d = dx.shape
    assert dy.is_contiguous() and dx.is_contiguous()
    _lib.check(lib.nm_time_bcast_add(_stream(), dy.data_ptr(), dx.data_ptr(), b, t, d), "nm_time_bcast_add")


def maxout_bwd(dy, argmax, dx, pool=2):
    lib = _lib.load()
    rows, groups, lddy = _rc(dy)
    _lib.check(lib.nm_maxout_bwd(_stream(), dy.data_ptr(), lddy, argmax.data_ptr(), dx.data_ptr(), _rc(dx)[2],
                                 rows, groups, pool), "nm_maxout_bwd")


def gru_gemm(mode, a, b, trans_b, t, ndir, rows, hsz, lengths=None, reverse_dir0=False, xp=None,
             x_strides=(0, 0, 0), h_in=None, h_out=None, ru=None, rh=None, c_save=None, out=None,
             out_strides=(0, 0, 0), dh=None, dout=None, dout_strides=(0, 0, 0), c=None, h0=None, hseq=None,
             hseq_strides=(0, 0, 0), dxp=None, dxp_strides=(0, 0, 0), dgpre=None, dcpre=None):
    """Recurrent GEMM of one GRU step with the fused epilogue ``mode`` (nm_gru_gemm).
    a: [ndir,R,K] (or [R,K]); b: [ndir,K,N] / [ndir,N,K] when trans_b (or 2-D for ndir == 1)."""
    lib = _lib.load()
    e = _lib.GruEpilogue()
    e.mode, e.t, e.rev_mask, e.ndir, e.R, e.H = mode, t, _rev_mask(ndir, reverse_dir0), ndir, rows, hsz
    e.lengths = _p(lengths)
    e.xp = _p(xp)
    e.x_dir, e.x_row, e.x_time = x_strides
    e.h_in, e.h_out, e.ru, e.rh, e.c_save, e.out = _p(h_in), _p(h_out), _p(ru), _p(rh), _p(c_save), _p(out)
    e.o_dir, e.o_row, e.o_time = out_strides
    e.dh, e.dout = _p(dh), _p(dout)
    e.do_dir, e.do_row, e.do_time = dout_strides
    e.c, e.h0, e.hseq = _p(c), _p(h0), _p(hseq)
    e.hs_dir, e.hs_row, e.hs_time = hseq_strides
    e.dxp = _p(dxp)
    e.dx_dir, e.dx_row, e.dx_time = dxp_strides
    e.dgpre, e.dcpre = _p(dgpre), _p(dcpre)
    a2 = a[0] if a.dim() == 3 else a
    b2 = b[0] if b.dim() == 3 else b
    assert a2.stride(1) == 1 and b2.stride(1) == 1
    k = a2.shape[1]
    s_a = a.stride(0) if a.dim() == 3 else 0
    s_b = b.stride(0) if b.dim() == 3 else 0
    _lib.check(lib.nm_gru_gemm(_stream(), ctypes.byref(e), int(trans_b), k, a.data_ptr(), a2.stride(0), s_a,
                               b.data_ptr(), b2.stride(0), s_b), "nm_gru_gemm")


def gru_seq_supported(rows, hsz, ndir) -> bool:
    """Can the time loops of this shape run as one cluster launch each (nm_gru_seq_fwd / nm_gru_seq_bwd)?"""
    return bool(_lib.load().nm_gru_seq_supported(rows, hsz, ndir))


def gru_seq_workspace_floats(rows, hsz, ndir) -> int:
    return _lib.load().nm_gru_seq_workspace_bytes(rows, hsz, ndir) // 4


def gru_seq_workspace(rows, hsz, ndir, device) -> torch.Tensor:
    """Header + granule buffers of one cluster loop (the call zeroes what it needs)."""
    return torch.empty(gru_seq_workspace_floats(rows, hsz, ndir), dtype=torch.float32, device=device)


def gru_seq_force_give_up(launches: int) -> int:
    """Test hook (nm_gru_seq_force_give_up): the next ``launches`` cluster loops behave like loops whose hand-offs
    timed out."""
    return int(_lib.load().nm_gru_seq_force_give_up(int(launches)))


def gru_seq_test_hog(blocks: int, lds_bytes: int, microseconds: int, stream=None) -> None:
    """Test utility (nm_gru_seq_test_hog): ``blocks`` workgroups that hold ``lds_bytes`` of LDS each for a while."""
    st = stream.cuda_stream if stream is not None else _stream()
    _lib.check(_lib.load().nm_gru_seq_test_hog(st, int(blocks), int(lds_bytes), int(microseconds)), "nm_gru_seq_test_hog")


def gru_seq_failed(workspace) -> bool:
    """After a synchronisation: did a cluster loop that used ``workspace`` give up waiting for a hand-off?"""
    return _lib.load().nm_gru_seq_failed(workspace.data_ptr()) != 0


# One cluster loop at a time per device.  A launch is ``ncu`` workgroups that must ALL be resident before they agree on
# their roles (csrc/nm_gru_cluster.hip); by registers exactly one such workgroup fits a CU (8 waves x 160 VGPRs = 2 per
# SIMD x 160 of 512), so two loops launched on two streams interleave over the CUs and neither becomes resident until
# both time out.  Every launch therefore waits for the previous one's event, whatever its stream, and leaves its own.
# Inside a stream capture the order is the captured stream's (a graph holds one loop after the other anyway).
_LAST_CLUSTER_LAUNCH = {}          # device index -> (event, stream it was recorded on)


def _cluster_serialize_before():
    if not torch.cuda.is_available() or torch.cuda.is_current_stream_capturing():
        return None
    stream = torch.cuda.current_stream()
    last = _LAST_CLUSTER_LAUNCH.get(stream.device.index)
    if last is not None and last[1] != stream.cuda_stream:
        stream.wait_event(last[0])
    return stream


def _cluster_serialize_after(stream):
    if stream is None:
        return
    last = _LAST_CLUSTER_LAUNCH.get(stream.device.index)
    event = last[0] if last is not None else torch.cuda.Event()
    event.record(stream)
    _LAST_CLUSTER_LAUNCH[stream.device.index] = (event, stream.cuda_stream)


def _cluster_call(name, *args):
    """Entry point ``name`` of a cluster loop on the current stream, inside the bracket above: the only way the
    wrappers below reach the library (a loop launched outside the bracket and another stream's loop can keep each
    other from becoming resident)."""
    serial = _cluster_serialize_before()
    _lib.check(getattr(_lib.load(), name)(_stream(), *args), name)
    _cluster_serialize_after(serial)


def _dir_strides(w):
    """(leading dimension, stride between directions) of a kernel [ndir, K, N], or [K, N] for one direction"""
    w2 = w[0] if w.dim() == 3 else w
    assert w2.stride(1) == 1
    return w2.stride(0), (w.stride(0) if w.dim() == 3 else 0)


def _seq_kernel(w):
    return (w.data_ptr(),) + _dir_strides(w)


def _seq_workspace(workspace, sticky):
    return workspace.data_ptr(), workspace.numel() * workspace.element_size(), _p(sticky)


def _seq_epilogue(mode, ndir, rows, hsz, lengths, reverse_dir0):
    """What the epilogues of all six loops share; the operands are the caller's."""
    e = _lib.GruEpilogue()
    e.mode, e.t, e.rev_mask, e.ndir, e.R, e.H = mode, 0, _rev_mask(ndir, reverse_dir0), ndir, rows, hsz
    e.lengths = _p(lengths)
    return e


def _seq_fwd_epilogue(ndir, rows, hsz, lengths, reverse_dir0, xp, x_strides, h_in0, h_out0, out, out_strides):
    e = _seq_epilogue(1, ndir, rows, hsz, lengths, reverse_dir0)
    e.xp = xp.data_ptr()
    e.x_dir, e.x_row, e.x_time = x_strides
    e.h_in, e.h_out, e.out = _p(h_in0), h_out0.data_ptr(), _p(out)
    e.o_dir, e.o_row, e.o_time = out_strides
    return e


def _seq_bwd_epilogue(ndir, rows, hsz, lengths, reverse_dir0, dh, dout, dout_strides, dxp, dxp_strides, h0=None,
                      hseq=None, hseq_strides=(0, 0, 0)):
    e = _seq_epilogue(4, ndir, rows, hsz, lengths, reverse_dir0)
    e.dh, e.dout = dh.data_ptr(), _p(dout)
    e.do_dir, e.do_row, e.do_time = dout_strides or (0, 0, 0)
    e.dxp = dxp.data_ptr()
    e.dx_dir, e.dx_row, e.dx_time = dxp_strides
    e.h0, e.hseq = _p(h0), _p(hseq)
    e.hs_dir, e.hs_row, e.hs_time = hseq_strides
    return e


def gru_seq_fwd(steps, ndir, rows, hsz, xp, x_strides, h_in0, h_out0, h_step, ru0, ru_step, rh0, rh_step, c0,
                c_step, wgh, wch, workspace, lengths=None, reverse_dir0=False, out=None, out_strides=(0, 0, 0),
                sticky=None, zero_padded=False, final=None, hprev_seq=None, rh_seq=None, seq_strides=None, h0_out=None):
    """All ``steps`` forward GRU steps in one launch (nm_gru_seq_fwd: workgroup clusters, csrc/nm_gru_cluster.hip).
    Tensors of step t: h_out0 + t*h_step etc. (element strides); ``rh0`` may be None; wgh [ndir,H,2H], wch [ndir,H,H]
    (2-D accepted for ndir 1); ``workspace`` from ``gru_seq_workspace``; ``sticky``: an int32 device word that a launch
    which gave up waiting sets to 1 (runtime.Session.error_word).

    What the loop does itself when asked (nm_gru_seq_fwd_ex): ``h_in0`` None: h_0 = 0; ``zero_padded``: zeros at the
    positions of ``out`` past a row's length; ``final`` [R, ndir*H] (row stride free): the state after each row's last
    valid step; ``hprev_seq`` / ``rh_seq`` with ``seq_strides`` (dir, row, time): h_{t-1} and r * h_{t-1} by position,
    zeros when padded; ``h0_out`` [ndir,R,H]: a copy of the initial state."""
    io = None
    if h_in0 is None or zero_padded or final is not None or hprev_seq is not None or rh_seq is not None or \
            h0_out is not None:
        io = _lib.GruSeqIo()
        io.zero_padded = int(bool(zero_padded))
        if final is not None:
            assert final.dim() == 2 and final.stride(1) == 1
            io.final_state, io.final_row, io.final_dir = final.data_ptr(), final.stride(0), hsz
        io.hprev_seq, io.rh_seq = _p(hprev_seq), _p(rh_seq)
        io.seq_dir, io.seq_row, io.seq_time = seq_strides or (0, 0, 0)
        io.h0_out = _p(h0_out)
    e = _seq_fwd_epilogue(ndir, rows, hsz, lengths, reverse_dir0, xp, x_strides, h_in0, h_out0, out, out_strides)
    e.ru, e.rh, e.c_save = ru0.data_ptr(), _p(rh0), _p(c0)
    tail = (steps, h_step, ru_step, rh_step, c_step, *_seq_kernel(wgh), *_seq_kernel(wch),
            *_seq_workspace(workspace, sticky))
    if io is None:
        _cluster_call("nm_gru_seq_fwd", ctypes.byref(e), *tail)
    else:
        _cluster_call("nm_gru_seq_fwd_ex", ctypes.byref(e), ctypes.byref(io), *tail)


def gru_seq_bwd(steps, ndir, rows, hsz, dh, dout, dout_strides, ru0, ru_step, c0, c_step, h0, hseq, hseq_strides,
                dxp, dxp_strides, wgh, wch, workspace, lengths=None, reverse_dir0=False, sticky=None, fused_io=False,
                d_final=None, d_final_dir=None, zero_padded=False):
    """The whole BPTT loop in one launch (nm_gru_seq_bwd): ``dh`` [ndir,R,H] holds dL/dh after the last step on entry
    and dL/dh_0 on exit; ``ru0`` / ``c0`` are the gates / candidates of step 0 (step t at + t*step elements);
    pre-activation gradients land in ``dxp``; wgh [ndir,H,2H], wch [ndir,H,H] (2-D accepted for ndir 1).

    ``fused_io`` (nm_gru_seq_bwd_ex): dL/dh after the last step is ``d_final`` [R, ndir*H] (row stride free; None: zero)
    and ``dh`` is only written (``d_final_dir``: element offset of a direction's block, default H); ``zero_padded``: zeros at the positions of ``dxp`` past a row's length."""
    io = None
    if fused_io:
        io = _lib.GruSeqIo()
        io.zero_padded = int(bool(zero_padded))
        if d_final is not None:
            assert d_final.dim() == 2 and d_final.stride(1) == 1
            io.d_final, io.dfinal_row = d_final.data_ptr(), d_final.stride(0)
            io.dfinal_dir = hsz if d_final_dir is None else d_final_dir
    else:
        assert d_final is None and not zero_padded
    e = _seq_bwd_epilogue(ndir, rows, hsz, lengths, reverse_dir0, dh, dout, dout_strides, dxp, dxp_strides, h0, hseq,
                          hseq_strides)
    e.ru, e.c = ru0.data_ptr(), c0.data_ptr()
    tail = (steps, ru_step, c_step, *_seq_kernel(wgh), *_seq_kernel(wch), *_seq_workspace(workspace, sticky))
    if io is None:
        _cluster_call("nm_gru_seq_bwd", ctypes.byref(e), *tail)
    else:
        _cluster_call("nm_gru_seq_bwd_ex", ctypes.byref(e), ctypes.byref(io), *tail)


def lstm_seq_workspace_floats(rows, hsz, ndir) -> int:
    return _lib.load().nm_lstm_seq_workspace_bytes(rows, hsz, ndir) // 4


def lstm_seq_supported(rows, hsz, ndir) -> bool:
    """Do the LSTM loops take this shape as one cluster launch each (nm_lstm_seq_fwd / nm_lstm_seq_bwd)?  The LSTM
    kernels' own answer: for a shape they do not take their workspace is the bare header (what no shape at all gets)."""
    lib = _lib.load()
    return lib.nm_lstm_seq_workspace_bytes(rows, hsz, ndir) > lib.nm_lstm_seq_workspace_bytes(0, 0, 0)


def lstm_seq_fwd(steps, ndir, rows, hsz, xp, x_strides, h_in0, h_out0, h_step, gates0, g_step, c0, c_step, wh, workspace,
                 forget_bias=1.0, lengths=None, reverse_dir0=False, out=None, out_strides=(0, 0, 0), sticky=None):
    """All ``steps`` forward steps of an LSTMCell layer in one launch (nm_lstm_seq_fwd).  ``xp`` 4H wide per direction
    (i | j | f | o), ``wh`` [ndir,H,4H]: the state half of the kernel, ``gates0`` / ``c0``: where step 0's activated gates
    and cell state are saved (step t at + t * step elements); zero initial cell state."""
    e = _seq_fwd_epilogue(ndir, rows, hsz, lengths, reverse_dir0, xp, x_strides, h_in0, h_out0, out, out_strides)
    e.ru, e.c_save = gates0.data_ptr(), c0.data_ptr()
    _cluster_call("nm_lstm_seq_fwd", ctypes.byref(e), steps, h_step, g_step, c_step, *_seq_kernel(wh),
                  float(forget_bias), *_seq_workspace(workspace, sticky))


def lstm_seq_bwd(steps, ndir, rows, hsz, dh, dout, dout_strides, gates0, g_step, c0, c_step, dxp, dxp_strides, wh,
                 workspace, lengths=None, reverse_dir0=False, sticky=None):
    """The BPTT loop of an LSTMCell layer in one launch (nm_lstm_seq_bwd): ``dh`` [ndir,R,H] holds dL/dh after the last
    step on entry and dL/dh_0 on exit; ``dxp`` (4H wide per direction) receives the pre-activation gradients."""
    e = _seq_bwd_epilogue(ndir, rows, hsz, lengths, reverse_dir0, dh, dout, dout_strides, dxp, dxp_strides)
    e.ru, e.c = gates0.data_ptr(), c0.data_ptr()
    _cluster_call("nm_lstm_seq_bwd", ctypes.byref(e), steps, g_step, c_step, *_seq_kernel(wh),
                  *_seq_workspace(workspace, sticky))


def nematus_seq_workspace_floats(rows, hsz, ndir) -> int:
    return _lib.load().nm_nematus_seq_workspace_bytes(rows, hsz, ndir) // 4


def nematus_seq_fwd(steps, ndir, rows, hsz, xp, x_strides, h_in0, h_out0, h_step, ru0, ru_step, sc0, sc_step, c0,
                    c_step, ug, uc, workspace, bgs=None, bcs=None, lengths=None, reverse_dir0=False, out=None,
                    out_strides=(0, 0, 0), sticky=None):
    """All ``steps`` forward steps of a NematusGRUCell layer in one launch (nm_nematus_seq_fwd).  As ``gru_seq_fwd``;
    ``ug`` [ndir,H,2H] / ``uc`` [ndir,H,H]: the state projections, ``bgs`` [ndir,2H] / ``bcs`` [ndir,H] their biases,
    ``sc0``: where step 0's h.U_c + b_cs is saved."""
    e = _seq_fwd_epilogue(ndir, rows, hsz, lengths, reverse_dir0, xp, x_strides, h_in0, h_out0, out, out_strides)
    e.ru, e.rh, e.c_save = ru0.data_ptr(), sc0.data_ptr(), c0.data_ptr()
    _cluster_call("nm_nematus_seq_fwd", ctypes.byref(e), steps, h_step, ru_step, sc_step, c_step, *_seq_kernel(ug),
                  *_seq_kernel(uc), _p(bgs), _p(bcs), *_seq_workspace(workspace, sticky))


def nematus_seq_bwd(steps, ndir, rows, hsz, dh, dout, dout_strides, ru0, ru_step, sc0, sc_step, c0, c_step, h0, hseq,
                    hseq_strides, dxp, dxp_strides, ug, uc, workspace, lengths=None, reverse_dir0=False, sticky=None):
    """The BPTT loop of a NematusGRUCell layer in one launch (nm_nematus_seq_bwd); ``dxp`` is 4H wide per direction:
    [dr' | du' | dc' | dsc]."""
    e = _seq_bwd_epilogue(ndir, rows, hsz, lengths, reverse_dir0, dh, dout, dout_strides, dxp, dxp_strides, h0, hseq,
                          hseq_strides)
    e.ru, e.rh, e.c = ru0.data_ptr(), sc0.data_ptr(), c0.data_ptr()
    _cluster_call("nm_nematus_seq_bwd", ctypes.byref(e), steps, ru_step, sc_step, c_step, *_seq_kernel(ug),
                  *_seq_kernel(uc), *_seq_workspace(workspace, sticky))


def optimizer_chunk_table(store, regularizable, trainable, cuts=(), chunk=65536):
    """The host side of the flat optimizer kernels' tables: every variable ("segment") is cut into chunks of at most
    ``chunk`` elements -- and at every flat offset in ``cuts`` (the slice boundaries of a sharded optimizer,
    distributed.ShardPlan.cuts: a chunk never straddles one, so every rank owns whole chunks).  The table -- and with it
    the order of every reduction -- depends on the cuts only, not on who owns which slice: one process and N ranks that
    use the same cuts compute bit-identical norms.  Returns (starts, lens, segs, seg_first, seg_count, seg_flags)."""
    import bisect
    cuts = sorted(set(int(c) for c in cuts))
    starts, lens, segs, first, count, flags = [], [], [], [], [], []
    for si, (name, spec) in enumerate(store.specs.items()):
        first.append(len(starts))
        off = 0
        while off < spec.size:
            n = min(chunk, spec.size - off)
            if cuts:
                k = bisect.bisect_right(cuts, spec.offset + off)
                if k < len(cuts) and cuts[k] < spec.offset + off + n:
                    n = cuts[k] - (spec.offset + off)
            starts.append(spec.offset + off)
            lens.append(n)
            segs.append(si)
            off += n
        count.append(len(starts) - first[-1])
        flags.append((1 if name in regularizable else 0) | (2 if name in trainable else 0))
    return starts, lens, segs, first, count, flags


def chunk_range_of(starts, lens, lo, hi):
    """The chunks whose elements lie in [lo, hi) of the flat buffer: (begin, end).  No chunk may straddle either end
    (the table was cut there: ``optimizer_chunk_table(..., cuts)``); the ends themselves may fall into the padding
    between two variables, which belongs to no chunk."""
    import bisect
    b, e = bisect.bisect_left(starts, lo), bisect.bisect_left(starts, hi)
    assert (b == 0 or starts[b - 1] + lens[b - 1] <= lo) and (e == 0 or starts[e - 1] + lens[e - 1] <= hi), \
        "a chunk straddles the end of a slice: the table was not cut there"
    return b, e


class OptimizerTables:
    """Chunk / segment tables of a VariableStore for the flat optimizer kernels."""
    CHUNK = 65536

    def __init__(self, store, regularizable, trainable, cuts=()):
        lib = _lib.load()
        self.names = list(store.specs)
        starts, lens, segs, first, count, flags = optimizer_chunk_table(store, regularizable, trainable, cuts, self.CHUNK)
        dev = store.device
        self._starts_host, self._lens_host = list(starts), list(lens)
        self.chunk_start = torch.tensor(starts, dtype=torch.int64, device=dev)
        self.chunk_len = torch.tensor(lens, dtype=torch.int32, device=dev)
        self.chunk_seg = torch.tensor(segs, dtype=torch.int32, device=dev)
        self.seg_first = torch.tensor(first, dtype=torch.int32, device=dev)
        self.seg_count = torch.tensor(count, dtype=torch.int32, device=dev)
        self.seg_flags = torch.tensor(flags, dtype=torch.int32, device=dev)
        self.nchunk, self.nseg = len(starts), len(first)
        self.workspace = torch.empty(lib.nm_optim_workspace_bytes(self.nchunk, self.nseg) // 4,
                                     dtype=torch.float32, device=dev)
        self.l1l2 = torch.zeros(2, dtype=torch.float32, device=dev)

    def _tabs(self):
        return (self.chunk_start.data_ptr(), self.chunk_len.data_ptr(), self.chunk_seg.data_ptr(),
                self.seg_first.data_ptr(), self.seg_count.data_ptr(), self.seg_flags.data_ptr(),
                self.nchunk, self.nseg)

    def regularize_and_norms(self, theta, grad, l1_weight, l2_weight):
        """grad += d(l1*L1 + l2*L2); per-variable ||grad||^2; returns device [L1, L2]."""
        lib = _lib.load()
        _lib.check(lib.nm_optim_regularize_norms(_stream(), theta.data_ptr(), grad.data_ptr(), *self._tabs(),
                                                 float(l1_weight), float(l2_weight), self.l1l2.data_ptr(),
                                                 self.workspace.data_ptr(), self.workspace.numel() * 4),
                   "nm_optim_regularize_norms")
        return self.l1l2

    def clip_adam(self, theta, grad, m, v, clip_norm, lr_t, beta1, beta2, epsilon, skip=None, chunks=None):
        """Per-tensor clip + Adam.  ``skip``: an int32 device word that, when not zero, turns the launch into a no-op
        (the session's error word: the update of a step whose time loop gave up is never applied); ``chunks``: the
        (begin, end) range of chunks a rank owns under the sharded optimizer (default: all)."""
        self.apply(0, theta, grad, m, v, clip_norm, (lr_t, beta1, beta2, epsilon), skip=skip, chunks=chunks)

    def clip_adadelta(self, theta, grad, accum, accum_update, clip_norm, lr, rho, epsilon, skip=None, chunks=None):
        self.apply(1, theta, grad, accum, accum_update, clip_norm, (lr, rho, epsilon, 0.0), skip=skip, chunks=chunks)

    def chunk_list(self, ranges):
        """Device int32 array of the chunk indices in the (begin, end) ``ranges`` (kept: a rank's ranges never change)."""
        key = tuple((int(b), int(e)) for b, e in ranges)
        lists = self.__dict__.setdefault("_chunk_lists", {})
        hit = lists.get(key)
        if hit is None:
            idx = [c for b, e in key for c in range(b, e)]
            hit = lists[key] = torch.tensor(idx, dtype=torch.int32, device=self.workspace.device)
        return hit

    def apply(self, kind, theta, grad, slot0, slot1, clip_norm, params, skip=None, chunks=None, chunk_list=None):
        """Pass 3, per-tensor clip + update of ``kind`` (optimizers.Optimizer.kind, with the four scalars of its
        ``params``): nm_optim_apply for kinds 0 and 1, nm_optim_update for 2..5, whose missing slots are ``None``.
        ``chunks``: a (begin, end) range (default: all), ``chunk_list``: a device list of chunk indices
        (``chunk_list()``) in one launch."""
        name = (("nm_optim_apply", "nm_optim_apply_list"),
                ("nm_optim_update", "nm_optim_update_list"))[int(kind) >= 2][chunk_list is not None]
        _lib.check(getattr(_lib.load(), name)(_stream(), int(kind), theta.data_ptr(), grad.data_ptr(), _p(slot0), _p(slot1),
                                              *self._tabs(), float(clip_norm or 0.0), *(float(x) for x in params),
                                              *self._select(chunks, chunk_list), _p(skip), self.workspace.data_ptr(),
                                              self.workspace.numel() * 4), name)

    def _select(self, chunks, chunk_list):
        """The pair of arguments that names a launch's chunks: a device list and its length, or a range's two ends."""
        if chunk_list is not None:
            return chunk_list.data_ptr(), chunk_list.numel()
        c0, c1 = chunks if chunks is not None else (0, self.nchunk)
        return int(c0), int(c1)

    def partials(self, theta, grad, l1_weight, l2_weight, chunks, chunk_list=None):
        """Pass 1 over the chunks [begin, end) -- or over a device list of chunks: regulariser terms into ``grad``,
        partial sums into the workspace."""
        name = ("nm_optim_partials", "nm_optim_partials_list")[chunk_list is not None]
        _lib.check(getattr(_lib.load(), name)(_stream(), theta.data_ptr(), grad.data_ptr(), *self._tabs(),
                                              float(l1_weight), float(l2_weight), *self._select(chunks, chunk_list),
                                              self.workspace.data_ptr(), self.workspace.numel() * 4), name)

    def partial_vector(self):
        """The 3 floats per chunk that ``partials`` writes (a view of the workspace)."""
        return self.workspace[:3 * self.nchunk]

    def segments(self):
        """Pass 2: per-variable squared norms + [L1, L2] from the whole partial vector, in a fixed order."""
        lib = _lib.load()
        _lib.check(lib.nm_optim_segments(_stream(), *self._tabs(), self.l1l2.data_ptr(), self.workspace.data_ptr(),
                                         self.workspace.numel() * 4), "nm_optim_segments")
        return self.l1l2

    def chunk_range(self, lo, hi):
        """The chunks whose elements lie in [lo, hi) of the flat buffer: (begin, end)."""
        return chunk_range_of(self._starts_host, self._lens_host, lo, hi)


# ---- sentence CNN encoder (csrc/nm_conv.hip) ------------------------------------------------------------------------
def _conv_tables(weights):
    """(widths, counts, pointer table) of filters W_i [w_i, E, n_i] as host arrays for the conv entry points."""
    n = len(weights)
    for w in weights:
        _f32(w)
        assert w.dim() == 3 and w.is_contiguous(), "conv filters are contiguous [w, E, n]"
    widths = (ctypes.c_int * n)(*[int(w.shape[0]) for w in weights])
    counts = (ctypes.c_int * n)(*[int(w.shape[2]) for w in weights])
    return widths, counts, (ctypes.c_void_p * n)(*[w.data_ptr() for w in weights])


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def conv1d_pool_shape(slen: int, segment: int):
    """(S', pad before) of the SAME max-pool over ``segment`` positions with stride ``segment``."""
    sp = (slen + segment - 1) // segment
    return sp, (sp * segment - slen) // 2


def conv1d_pool_fwd(x, weights, biases, segment, pooled, argmax, mask=None, lengths=None, mask_out=None,
                    seq_lens=None, algo=0):
    """pooled [B, S', sum n_i] (+ int32 argmax) = per width max-pool(relu(conv1d_SAME(x [B, S, E], W_i) + b_i)), all
    widths in one launch (nm_conv1d_pool_fwd); optionally the pooled mask [B, S'] and ceil(lengths / segment)."""
    lib = _lib.load()
    _f32(x), _f32(pooled), _i32(argmax)
    bsz, slen, e = x.shape
    assert x.stride(2) == 1 and x.stride(0) == slen * x.stride(1), "x: [B, S, E] rows of one stride"
    assert pooled.is_contiguous() and argmax.is_contiguous() and pooled.shape == argmax.shape
    widths, counts, wtab = _conv_tables(weights)
    assert all(_f32(b).is_contiguous() and b.numel() == w.shape[2] for b, w in zip(biases, weights))
    if mask is not None:
        assert mask.is_contiguous() and mask_out is not None and mask_out.is_contiguous()
    _lib.check(lib.nm_conv1d_pool_fwd(_stream(), x.data_ptr(), x.stride(1), bsz, slen, e, int(segment), len(weights),
                                      widths, counts, wtab, _ptrs(biases), pooled.data_ptr(), argmax.data_ptr(),
                                      pooled.shape[-1], _p(mask), _p(lengths), _p(mask_out), _p(seq_lens), int(algo)),
               "nm_conv1d_pool_fwd")
    return pooled, argmax


def conv1d_wgrad_workspace_floats(bsz, slen, e, weights) -> int:
    widths, counts, _ = _conv_tables(weights)
    return int(_lib.load().nm_conv1d_wgrad_workspace_bytes(bsz, slen, e, len(weights), widths, counts)) // 4


def conv1d_pool_bwd(x, weights, segment, pooled, argmax, dpooled, dz, dx=None, accumulate_dx=False, dweights=None,
                    dbiases=None, accumulate_params=True, workspace=None, algo=0):
    """The gradient of ``conv1d_pool_fwd``: dz [B, S, sum n_i] (scratch, written whole) = dpooled at the argmax where
    pooled > 0; dx (+)= the transposed convolution of every width; dW_i / db_i (+)= the filter / bias gradients
    (nm_conv1d_pool_bwd; deterministic).  ``workspace``: conv1d_wgrad_workspace_floats floats."""
    lib = _lib.load()
    bsz, slen, e = x.shape
    assert x.stride(2) == 1 and x.stride(0) == slen * x.stride(1)
    assert dpooled.is_contiguous() and dz.is_contiguous() and dz.shape[-1] == pooled.shape[-1]
    assert dx is None or (dx.stride(1) == x.stride(1) and dx.stride(0) == x.stride(0) and dx.stride(2) == 1)
    widths, counts, wtab = _conv_tables(weights)
    dw_tab = db_tab = None
    if dweights is not None:
        assert all(g.is_contiguous() and g.shape == w.shape for g, w in zip(dweights, weights))
        dw_tab, db_tab = _ptrs(dweights), _ptrs(dbiases)
    _lib.check(lib.nm_conv1d_pool_bwd(_stream(), x.data_ptr(), x.stride(1), bsz, slen, e, int(segment), len(weights),
                                      widths, counts, wtab, pooled.data_ptr(), argmax.data_ptr(), dpooled.data_ptr(),
                                      pooled.shape[-1], dz.data_ptr(), _p(dx), int(accumulate_dx), dw_tab, db_tab,
                                      int(accumulate_params), _p(workspace),
                                      0 if workspace is None else workspace.numel() * 4, int(algo)),
               "nm_conv1d_pool_bwd")


def highway_fwd(zt, zh, x, bt, bh, y, tsave, hsave):
    """y = relu(zh + bh) T + x (1 - T), T = sigmoid(zt + bt) (nm_highway_fwd); T, H kept for the backward pass."""
    rows, cols, ldx = _rc(x)
    assert _rc(y)[2] == ldx and _rc(zh)[2] == _rc(zt)[2] and tsave.is_contiguous() and hsave.is_contiguous()
    if rows == 0:                     # (an empty tensor has a null data pointer, which the entry point refuses)
        return y
    _lib.check(_lib.load().nm_highway_fwd(_stream(), zt.data_ptr(), zh.data_ptr(), _rc(zt)[2], x.data_ptr(), ldx,
                                          bt.data_ptr(), bh.data_ptr(), y.data_ptr(), tsave.data_ptr(),
                                          hsave.data_ptr(), rows, cols), "nm_highway_fwd")
    return y


def highway_bwd(dy, x, tsave, hsave, dzt, dzh, dx, accumulate_dx=False):
    """dzt, dzh (the gradients of the two products' outputs) and the carry term of dx (nm_highway_bwd)."""
    rows, cols, ldx = _rc(x)
    assert _rc(dy)[2] == ldx and _rc(dx)[2] == ldx and _rc(dzh)[2] == _rc(dzt)[2]
    if rows == 0:
        return
    _lib.check(_lib.load().nm_highway_bwd(_stream(), dy.data_ptr(), x.data_ptr(), ldx, tsave.data_ptr(),
                                          hsave.data_ptr(), dzt.data_ptr(), dzh.data_ptr(), _rc(dzt)[2], dx.data_ptr(),
                                          rows, cols, int(accumulate_dx)), "nm_highway_bwd")


# ---- ConvS2S residual layer (include/nmhip_convs2s.h, csrc/nm_conv.hip) -------------------------------------------------
def conv1d_glu_workspace_floats(bsz, steps, c, width) -> int:
    """Floats of the workspace ``conv1d_glu_bwd`` needs for the weight gradient of this shape."""
    return int(_lib.load().nm_conv1d_glu_workspace_bytes(bsz, steps, c, width)) // 4


def conv1d_glu_fwd(x, filt, bias, y, lin_save=None, sig_save=None, algo=0):
    """y [B, T, C] = glu(conv1d_SAME(x [B, T, C], filt [w, C, 2C]) + bias [2C]) + x in one launch (nm_conv1d_glu_fwd);
    ``lin_save`` / ``sig_save`` [B*T, C]: what ``conv1d_glu_bwd`` reads, both or neither."""
    bsz, steps, c, ldx = _btd(x, "conv1d_glu_fwd x")
    assert tuple(y.shape) == (bsz, steps, c)
    ldy = _btd(y, "conv1d_glu_fwd y")[3]
    _f32(filt), _f32(bias)
    assert filt.dim() == 3 and filt.is_contiguous() and tuple(filt.shape[1:]) == (c, 2 * c), "filter [w, C, 2C]"
    assert bias.is_contiguous() and bias.numel() == 2 * c
    for save in (lin_save, sig_save):
        assert save is None or (_f32(save).is_contiguous() and save.numel() == bsz * steps * c)
    _lib.check(_lib.load().nm_conv1d_glu_fwd(_stream(), x.data_ptr(), ldx, bsz, steps, c, int(filt.shape[0]),
                                             filt.data_ptr(), bias.data_ptr(), y.data_ptr(), ldy, _p(lin_save),
                                             _p(sig_save), int(algo)), "nm_conv1d_glu_fwd")
    return y


def conv1d_glu_bwd(x, filt, lin_save, sig_save, dy, dz, dx=None, accumulate_dx=False, dfilt=None, dbias=None,
                   accumulate_params=True, workspace=None, algo=0):
    """The gradient of ``conv1d_glu_fwd``: dz [B*T, 2C] (scratch, written whole); dx (+)= dy + conv^T(dz, filt);
    dfilt / dbias (+)= the filter / bias gradients (nm_conv1d_glu_bwd; deterministic).  ``workspace``:
    conv1d_glu_workspace_floats floats, needed with ``dfilt``."""
    bsz, steps, c, ldx = _btd(x, "conv1d_glu_bwd x")
    assert tuple(dy.shape) == (bsz, steps, c)
    lddy = _btd(dy, "conv1d_glu_bwd dy")[3]
    lddx = 0
    if dx is not None:
        assert tuple(dx.shape) == (bsz, steps, c)
        lddx = _btd(dx, "conv1d_glu_bwd dx")[3]
    _f32(filt)
    assert filt.dim() == 3 and filt.is_contiguous() and tuple(filt.shape[1:]) == (c, 2 * c), "filter [w, C, 2C]"
    assert _f32(dz).is_contiguous() and dz.numel() == bsz * steps * 2 * c
    assert lin_save.is_contiguous() and sig_save.is_contiguous() and lin_save.numel() == sig_save.numel() == bsz * steps * c
    assert dfilt is None or (_f32(dfilt).is_contiguous() and dfilt.shape == filt.shape)
    assert dbias is None or (_f32(dbias).is_contiguous() and dbias.numel() == 2 * c)
    _lib.check(_lib.load().nm_conv1d_glu_bwd(_stream(), x.data_ptr(), ldx, bsz, steps, c, int(filt.shape[0]),
                                             filt.data_ptr(), lin_save.data_ptr(), sig_save.data_ptr(), dy.data_ptr(),
                                             lddy, dz.data_ptr(), _p(dx), lddx, int(bool(accumulate_dx)), _p(dfilt),
                                             _p(dbias), int(bool(accumulate_params)), _p(workspace),
                                             0 if workspace is None else workspace.numel() * 4, int(algo)),
               "nm_conv1d_glu_bwd")


# ---- connectionist temporal classification (include/nmhip_ctc.h, csrc/nm_ctc.hip) -------------------------------------
_CTC_WS = {}


def ctc_workspace_bytes(bsz: int, steps: int, max_labels: int) -> int:
    return int(_lib.load().nm_ctc_workspace_bytes(bsz, steps, max_labels))


def ctc_workspace(bsz: int, steps: int, max_labels: int, device) -> torch.Tensor:
    """Persistent workspace of the CTC calls, one per (device, stream, workspace tag) like the GEMM's split-K slabs; it
    grows to the largest batch seen.  ``ctc_loss_bwd`` reads what ``ctc_loss_fwd`` left in it."""
    need = ctc_workspace_bytes(bsz, steps, max_labels)
    key = (device, _stream(), workspace_tag())
    ws = _CTC_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=device)
        _CTC_WS[key] = ws
    return ws


def _ctc_logits(logits):
    """logits [T, B, K] as any strided view with a unit class stride (a transposed batch-major product included)."""
    _f32(logits)
    assert logits.dim() == 3 and (logits.shape[2] == 1 or logits.stride(2) == 1), "unit class stride"
    return logits.shape[0], logits.shape[1], logits.shape[2]


def ctc_mask_lengths(mask, out=None):
    """int32 row sums of a 0/1 float mask [B, T] (TemporalStateful.lengths)."""
    _f32(mask)
    assert mask.dim() == 2 and (mask.shape[1] == 1 or mask.stride(1) == 1)
    if out is None:
        out = torch.empty(mask.shape[0], dtype=torch.int32, device=mask.device)
    _lib.check(_lib.load().nm_ctc_mask_lengths(_stream(), mask.data_ptr(), mask.stride(0), mask.shape[0], mask.shape[1],
                                               _i32(out).data_ptr()), "nm_ctc_mask_lengths")
    return out


def ctc_loss_fwd(logits, labels, label_len, frame_len, merge_repeated, loss, loss_sum, workspace=None):
    """loss [B] and their sum loss_sum [1] of tf.nn.ctc_loss over logits [T, B, K] (blank = K - 1); labels [B, Lmax]
    int32 with label_len [B] entries each, frame_len [B].  Returns the workspace ``ctc_loss_bwd`` needs."""
    steps, bsz, k = _ctc_logits(logits)
    assert labels.dim() == 2 and labels.shape[0] == bsz and (labels.numel() == 0 or labels.is_contiguous())
    assert label_len.numel() == bsz and frame_len.numel() == bsz and loss.numel() == bsz and loss.is_contiguous()
    lmax = labels.shape[1]
    if workspace is None:
        workspace = ctc_workspace(bsz, steps, lmax, logits.device)
    _lib.check(_lib.load().nm_ctc_loss_fwd(_stream(), logits.data_ptr(), logits.stride(0), logits.stride(1), steps, bsz, k,
                                           _i32(labels).data_ptr(), lmax, _i32(label_len).data_ptr(),
                                           _i32(frame_len).data_ptr(), int(bool(merge_repeated)), _f32(loss).data_ptr(),
                                           _f32(loss_sum).data_ptr(), workspace.data_ptr(), workspace.numel()),
               "nm_ctc_loss_fwd")
    return workspace


def ctc_loss_bwd(logits, labels, label_len, frame_len, dlogits, workspace, grad_scale=None):
    """dlogits = grad_scale[0] * (softmax(logits) - occupancy) after ``ctc_loss_fwd`` on the same operands; dlogits is
    a [T, B, K] view of its own (strides may differ) or the logits themselves."""
    steps, bsz, k = _ctc_logits(logits)
    assert tuple(dlogits.shape) == (steps, bsz, k) and _ctc_logits(dlogits)
    lmax = labels.shape[1]
    _lib.check(_lib.load().nm_ctc_loss_bwd(_stream(), logits.data_ptr(), logits.stride(0), logits.stride(1), steps, bsz, k,
                                           _i32(labels).data_ptr(), lmax, _i32(label_len).data_ptr(),
                                           _i32(frame_len).data_ptr(), _p(grad_scale), dlogits.data_ptr(),
                                           dlogits.stride(0), dlogits.stride(1), workspace.data_ptr(), workspace.numel()),
               "nm_ctc_loss_bwd")
    return dlogits


def ctc_greedy(logits, frame_len, merge_repeated, end_token, tokens, out_len, workspace=None):
    """tf.nn.ctc_greedy_decoder over logits [T, B, K]: tokens [B, T] int32 = the emitted classes of each sentence, then
    ``end_token``; out_len [B] = how many were emitted."""
    steps, bsz, k = _ctc_logits(logits)
    assert tuple(tokens.shape) == (bsz, steps) and (tokens.numel() == 0 or tokens.is_contiguous())
    assert out_len.numel() == bsz and frame_len.numel() == bsz
    if workspace is None:
        workspace = ctc_workspace(bsz, steps, 0, logits.device)
    _lib.check(_lib.load().nm_ctc_greedy(_stream(), logits.data_ptr(), logits.stride(0), logits.stride(1), steps, bsz, k,
                                         _i32(frame_len).data_ptr(), int(bool(merge_repeated)), int(end_token),
                                         _i32(tokens).data_ptr(), _i32(out_len).data_ptr(), workspace.data_ptr(),
                                         workspace.numel()), "nm_ctc_greedy")
    return tokens, out_len


# ---- sequence labelling (include/nmhip_label.h, csrc/nm_label.hip) ----------------------------------------------------
def label_rows_max_classes() -> int:
    return int(_lib.load().nm_label_rows_max_classes())


def label_rows(logits, targets=None, pad_id=0, grad_scale=None, write_grad=False, loss_rows=None, logprobs=None,
               argmax=None, row_mask=None, masked_class=0, labels=None):
    """The rows of a labelling head in one call (decoders/sequence_labeler.py:114-129): ``loss_rows`` [R] = cross
    entropy where ``targets`` [R] int32 differ from ``pad_id`` (exact zeros elsewhere), ``logprobs`` [R, K] =
    log_softmax, ``argmax`` [R] int32 (first maximum), ``labels`` [R] int32 = argmax where ``row_mask`` [R] is not zero,
    else ``masked_class``; with ``write_grad`` the logits [R, K] become grad_scale[0] * d sum(loss) / d logits in
    place.  One packed kernel up to ``label_rows_max_classes()`` classes; wider rows (an EmbeddingsLabeler over a
    translation vocabulary) go through the vocabulary-row kernels nm_row_stats / nm_log_softmax / nm_xent, with the
    same results."""
    lib = _lib.load()
    _f32(logits)
    assert logits.dim() == 2 and (logits.shape[1] == 1 or logits.stride(1) == 1), "unit class stride"
    rows, k = logits.shape
    ld = logits.stride(0) if rows > 1 else max(logits.stride(0), k)
    if write_grad and targets is None:
        raise ValueError("label_rows: write_grad needs targets")
    if labels is not None and row_mask is None:
        raise ValueError("label_rows: labels need a row_mask")
    for t, n in ((targets, "targets"), (argmax, "argmax"), (labels, "labels")):
        assert t is None or (_i32(t).numel() == rows and t.is_contiguous()), n
    for t, n in ((loss_rows, "loss_rows"), (row_mask, "row_mask")):
        assert t is None or (_f32(t).numel() == rows and t.is_contiguous()), n
    ldp = 0
    if logprobs is not None:
        _f32(logprobs)
        assert tuple(logprobs.shape) == (rows, k) and (k == 1 or logprobs.stride(1) == 1)
        ldp = logprobs.stride(0) if rows > 1 else max(logprobs.stride(0), k)
    if k <= label_rows_max_classes():
        _lib.check(lib.nm_label_rows(_stream(), logits.data_ptr(), ld, rows, k, _p(targets), int(pad_id), _p(grad_scale),
                                     int(bool(write_grad)), _p(loss_rows), _p(logprobs), ldp, _p(argmax), _p(row_mask),
                                     int(masked_class), _p(labels)), "nm_label_rows")
        return
    if rows == 0:
        return
    if logprobs is not None:                                       # (before anything is launched)
        x_end = logits.data_ptr() + 4 * ((rows - 1) * ld + k)
        p_end = logprobs.data_ptr() + 4 * ((rows - 1) * ldp + k)
        if not (p_end <= logits.data_ptr() or x_end <= logprobs.data_ptr()):         # the packed kernel's range test
            raise _lib.NMHipError("label_rows: logprobs aliasing logits")
    dev = logits.device
    want_stats = logprobs is not None or (targets is not None and loss_rows is not None)
    rmax = torch.empty(rows, dtype=torch.float32, device=dev) if want_stats else None
    rlse = torch.empty(rows, dtype=torch.float32, device=dev) if want_stats else None
    if argmax is None and labels is not None:
        argmax = torch.empty(rows, dtype=torch.int32, device=dev)
    if want_stats or argmax is not None:
        _lib.check(lib.nm_row_stats(_stream(), logits.data_ptr(), ld, rows, k, _p(rmax), _p(rlse), _p(argmax)),
                   "nm_row_stats")
    if logprobs is not None:
        _lib.check(lib.nm_log_softmax(_stream(), logits.data_ptr(), ld, rmax.data_ptr(), rlse.data_ptr(),
                                      logprobs.data_ptr(), ldp, rows, k), "nm_log_softmax")
    weights = torch.empty(rows, dtype=torch.float32, device=dev) if write_grad else None
    if targets is not None or labels is not None:
        _lib.check(lib.nm_label_rows_from_stats(_stream(), logits.data_ptr(), ld, rows, k, _p(targets), int(pad_id),
                                                _p(rmax), _p(rlse), _p(loss_rows), _p(weights), _p(argmax), _p(row_mask),
                                                int(masked_class), _p(labels)), "nm_label_rows_from_stats")
    if write_grad:            # the gradient alone: the loss above already holds the NaN / exact-zero conventions
        _lib.check(lib.nm_xent(_stream(), logits.data_ptr(), ld, rows, k, targets.data_ptr(), weights.data_ptr(), None,
                               _p(grad_scale), 1, 0.0), "nm_xent")


# ---- supervised attention (include/nmhip_align.h, csrc/nm_align.hip) ----------------------------------------------------
def _tbs(w, what):
    """(T, B, S) of dense time-major attention weights."""
    _f32(w)
    assert w.dim() == 3 and (w.numel() == 0 or w.is_contiguous()), what + ": dense [T, B, S]"
    return tuple(w.shape)


def align_xent(w, target, pad, loss_rows, scale=None, dw=None, accumulate=False):
    """The rows of WordAlignmentDecoder's training loss (decoders/word_alignment_decoder.py:100-108) in one launch:
    ``loss_rows`` [T, B] = pad * softmax_cross_entropy_with_logits(labels = target[b, t, :S], logits = w[t, b, :]) over the
    attention weights ``w`` [T, B, S]; with ``dw`` [T, B, S] also scale[0] * pad * (softmax(w) - label), TensorFlow's
    registered gradient, written or (``accumulate``) added.  ``target`` is the batch-major fed array [B, T', S'] with
    T' >= T and S' >= S, read in place through its strides: rows t >= T and columns s >= S are never read."""
    steps, bsz, slen = _tbs(w, "align_xent w")
    _f32(target)
    assert target.dim() == 3 and target.shape[0] == bsz and target.shape[1] >= steps and target.shape[2] >= slen, \
        (tuple(target.shape), (steps, bsz, slen))
    assert target.shape[2] == 1 or target.stride(2) == 1, "align_xent target: unit source stride"
    st = target.stride(1) if target.shape[1] > 1 else max(target.stride(1), target.shape[2])
    sb = target.stride(0) if bsz > 1 else max(target.stride(0), target.shape[1] * st)
    for t, n in ((pad, "pad"), (loss_rows, "loss_rows")):
        assert _f32(t).numel() == steps * bsz and (t.numel() == 0 or t.is_contiguous()), n
    if dw is not None:
        assert _tbs(dw, "align_xent dw") == (steps, bsz, slen)
    if scale is not None:
        assert _f32(scale).numel() == 1
    _lib.check(_lib.load().nm_align_xent(_stream(), w.data_ptr(), steps, bsz, slen, target.data_ptr(), sb, st,
                                         pad.data_ptr(), _p(scale), loss_rows.data_ptr(), _p(dw),
                                         int(bool(accumulate))), "nm_align_xent")
    return loss_rows


def align_softmax(w, out):
    """out [B, T, S] = softmax(w [T, B, S]) over the source positions, batch-major (word_alignment_decoder.py:91-97)."""
    steps, bsz, slen = _tbs(w, "align_softmax w")
    _f32(out)
    assert tuple(out.shape) == (bsz, steps, slen) and (out.numel() == 0 or out.is_contiguous())
    _lib.check(_lib.load().nm_align_softmax(_stream(), w.data_ptr(), steps, bsz, slen, out.data_ptr()),
               "nm_align_softmax")
    return out


# ---- the speech front end (include/nmhip_speech.h, csrc/nm_speech.hip) --------------------------------------------------
def _offsets(t, what):
    assert t.dtype == torch.int64 and t.is_cuda and t.dim() == 1 and t.numel() >= 2 and t.is_contiguous(), what
    return t.numel() - 1


def speech_frames(wav, sample_off, frame_off, frame_len, frame_step, nfft, preemph, tables, mode, numcep, append_energy,
                  out):
    """Feature block 0 of a ragged batch of utterances: ``wav`` holds their fp32 samples back to back, utterance u at
    ``sample_off[u] .. sample_off[u+1]``, its frames are the rows ``frame_off[u] .. frame_off[u+1]`` of ``out``
    [total_frames, ld].  ``tables``: the device tensors of ``processors.speech.SpeechTables.on_device``."""
    _f32(wav)
    _f32(out)
    count = _offsets(sample_off, "speech_frames sample_off")
    assert _offsets(frame_off, "speech_frames frame_off") == count
    assert wav.dim() == 1 and wav.is_contiguous() and out.dim() == 2 and (out.numel() == 0 or out.stride(1) == 1)
    nbins = nfft // 2 + 1
    bank, window, twiddles, ranges = tables["bank"], tables["window"], tables["twiddles"], tables["bank_range"]
    nfilt = bank.shape[0]
    assert _f32(bank).is_contiguous() and tuple(bank.shape) == (nfilt, nbins), tuple(bank.shape)
    assert _f32(window).is_contiguous() and window.numel() == frame_len
    assert _f32(twiddles).is_contiguous() and tuple(twiddles.shape) == (nfft // 2, 2)
    assert _i32(ranges).is_contiguous() and tuple(ranges.shape) == (nfilt, 2)
    dct, freqs = tables.get("dct"), tables.get("centroid_freqs")
    if dct is not None:
        assert _f32(dct).is_contiguous() and tuple(dct.shape) == (numcep, nfilt), tuple(dct.shape)
    if freqs is not None:
        assert _f32(freqs).is_contiguous() and freqs.numel() == nbins
    ld = out.stride(0) if out.shape[0] > 1 else out.shape[1]
    _lib.check(_lib.load().nm_speech_frames(_stream(), wav.data_ptr(), sample_off.data_ptr(), frame_off.data_ptr(), count,
                                            wav.numel(), out.shape[0], int(frame_len), int(frame_step), int(nfft),
                                            float(preemph), window.data_ptr(), twiddles.data_ptr(), bank.data_ptr(),
                                            ranges.data_ptr(), nfilt, _p(dct), int(numcep), _p(freqs), int(mode),
                                            int(bool(append_energy)), out.data_ptr(), ld), "nm_speech_frames")
    return out


def speech_deltas(out, frame_off, width, order, window):
    """One order of deltas: column block ``order + 1`` of ``out`` from block ``order`` (blocks ``width`` wide), rows
    clamped to their own utterance."""
    _f32(out)
    count = _offsets(frame_off, "speech_deltas frame_off")
    assert out.dim() == 2 and (out.numel() == 0 or out.stride(1) == 1)
    ld = out.stride(0) if out.shape[0] > 1 else out.shape[1]
    _lib.check(_lib.load().nm_speech_deltas(_stream(), out.data_ptr(), ld, frame_off.data_ptr(), count, out.shape[0],
                                            int(width), int(order), int(window)), "nm_speech_deltas")
    return out


# ---- the image reader's device pipeline (include/nmhip_imgread.h, csrc/nm_imgread.hip) ----------------------------------
IMGREAD_TARGETS = {"L": 0, "RGB": 1, "F": 2}
IMGREAD_OFFS, IMGREAD_GEOM = 6, 16


def _imgread_chunk(offs, geom, bounds, coef, target):
    """Checks the device arrays of one chunk (``readers.image_reader.ChunkPlan.arrays``); -> number of images."""
    assert offs.dtype == torch.int64 and offs.is_cuda and offs.is_contiguous() and offs.dim() == 2, "imgread offs"
    assert offs.shape[0] == IMGREAD_OFFS and offs.shape[1] >= 2, tuple(offs.shape)
    count = offs.shape[1] - 1
    assert _i32(geom).is_contiguous() and tuple(geom.shape) == (count, IMGREAD_GEOM), tuple(geom.shape)
    assert _i32(bounds).is_contiguous() and bounds.dim() == 2 and bounds.shape[1] == 2, tuple(bounds.shape)
    want = torch.float64 if target == IMGREAD_TARGETS["F"] else torch.int32
    assert coef.dtype == want and coef.is_cuda and coef.dim() == 1 and coef.is_contiguous(), (coef.dtype, want)
    return count


def imgread_rows(src, offs, geom, bounds, coef, target, pad_w, max_rows, scratch):
    """Horizontal pass of a chunk of decoded 8-bit images, the conversion to ``target`` folded into the loads: ``src``
    (uint8, the images back to back) -> ``scratch`` (uint8 for the targets L and RGB, float32 for F)."""
    count = _imgread_chunk(offs, geom, bounds, coef, target)
    assert src.dtype == torch.uint8 and src.is_cuda and src.dim() == 1 and src.is_contiguous()
    want = torch.float32 if target == IMGREAD_TARGETS["F"] else torch.uint8
    assert scratch.dtype == want and scratch.is_cuda and scratch.dim() == 1 and scratch.is_contiguous()
    _lib.check(_lib.load().nm_imgread_rows(_stream(), src.data_ptr(), src.numel(), offs.data_ptr(), geom.data_ptr(), count,
                                           bounds.data_ptr(), bounds.shape[0], coef.data_ptr(), coef.numel(), int(target),
                                           int(pad_w), int(max_rows), scratch.data_ptr(), scratch.numel()),
               "nm_imgread_rows")
    return scratch


def imgread_cols(scratch, offs, geom, bounds, coef, target, out, sub=None, divide=1.0):
    """Vertical pass, crop, zero padding and the optional ``(v - sub[c]) / divide`` epilogue: ``scratch`` -> ``out``
    [N, pad_h, pad_w, C] float32 (rows contiguous; images and rows may be strided alike)."""
    count = _imgread_chunk(offs, geom, bounds, coef, target)
    _f32(out)
    assert out.dim() == 4 and out.shape[0] == count and out.is_contiguous(), tuple(out.shape)
    channels = 3 if target == IMGREAD_TARGETS["RGB"] else 1
    assert out.shape[3] == channels, (tuple(out.shape), channels)
    if sub is not None:
        assert sub.dtype == torch.float64 and sub.is_cuda and sub.numel() == channels and sub.is_contiguous()
    _lib.check(_lib.load().nm_imgread_cols(_stream(), scratch.data_ptr(), scratch.numel(), offs.data_ptr(),
                                           geom.data_ptr(), count, bounds.data_ptr(), bounds.shape[0], coef.data_ptr(),
                                           coef.numel(), int(target), out.shape[2], out.shape[1], _p(sub), float(divide),
                                           out.data_ptr(), out.shape[2] * channels), "nm_imgread_cols")
    return out


def imgread_check(offs, geom, target, pad_w, pad_h):
    """The host copies (NumPy) of a chunk's offsets and geometry, checked before they are uploaded."""
    import numpy as np
    assert offs.dtype == np.int64 and offs.flags.c_contiguous and offs.ndim == 2 and offs.shape[0] == IMGREAD_OFFS
    assert geom.dtype == np.int32 and geom.flags.c_contiguous and geom.shape == (offs.shape[1] - 1, IMGREAD_GEOM)
    _lib.check(_lib.load().nm_imgread_check(offs.ctypes.data, geom.ctypes.data, geom.shape[0], int(target), int(pad_w),
                                            int(pad_h)), "nm_imgread_check")


# ---- sentence-level heads (include/nmhip_pool.h, csrc/nm_pool.hip) ------------------------------------------------------
POOL_MODES = {"max": 0, "avg": 1}


def _btd(x, what):
    """(B, T, D, row stride) of batch-major states [B, T, D] whose (b, t) rows lie one row stride apart."""
    _f32(x)
    assert x.dim() == 3, what
    bsz, steps, d = x.shape
    assert d == 1 or x.stride(2) == 1, what + ": unit feature stride"
    ld = x.stride(1) if steps > 1 else max(x.stride(1), d)
    assert bsz == 1 or x.stride(0) == steps * ld, what + ": batch-major rows one row stride apart"
    return bsz, steps, d, ld


def _ld2(t, cols, what):
    _f32(t)
    assert t.dim() == 2 and t.shape[1] == cols and (cols == 1 or t.stride(1) == 1), what
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), cols)


def pool_fwd(mode, x, mask, out, ties=None):
    """Masked max / average over time of [B, T, D] states (encoders/pooling.py): ``out`` [B, D]; with "max" also
    ``ties`` [B, D] int32, how many of the T positions equal the maximum."""
    bsz, steps, d, ldx = _btd(x, "pool_fwd x")
    assert tuple(mask.shape) == (bsz, steps) and _f32(mask).is_contiguous()
    assert out.shape[0] == bsz
    ldo = _ld2(out, d, "pool_fwd out")
    if ties is not None:
        assert tuple(_i32(ties).shape) == (bsz, d) and ties.is_contiguous()
    _lib.check(_lib.load().nm_pool_fwd(_stream(), POOL_MODES[mode], x.data_ptr(), ldx, mask.data_ptr(), bsz, steps, d,
                                       out.data_ptr(), ldo, _p(ties)), "nm_pool_fwd")
    return out


def pool_bwd(mode, dout, mask, dx, x=None, out=None, ties=None, accumulate=False):
    """dx (+)= the gradient of ``pool_fwd``; every (b, t, d) is written, padded positions with exact zeros.  "max" needs
    ``x``, ``out`` and ``ties`` of the forward call."""
    bsz, steps, d, lddx = _btd(dx, "pool_bwd dx")
    assert tuple(mask.shape) == (bsz, steps) and _f32(mask).is_contiguous()
    assert dout.shape[0] == bsz
    lddo = _ld2(dout, d, "pool_bwd dout")
    ldx = ldo = 0
    if x is not None:
        assert tuple(x.shape) == (bsz, steps, d)
        ldx = _btd(x, "pool_bwd x")[3]
    if out is not None:
        assert out.shape[0] == bsz
        ldo = _ld2(out, d, "pool_bwd out")
    if ties is not None:
        assert tuple(_i32(ties).shape) == (bsz, d) and ties.is_contiguous()
    _lib.check(_lib.load().nm_pool_bwd(_stream(), POOL_MODES[mode], _p(x), ldx, mask.data_ptr(), _p(out), ldo, _p(ties),
                                       dout.data_ptr(), lddo, bsz, steps, d, dx.data_ptr(), lddx, int(bool(accumulate))),
               "nm_pool_bwd")
    return dx


def split_mask(mask, factor, out_mask, lengths):
    """model/sequence_split.py: ``out_mask`` [B, T*factor] = every entry of ``mask`` [B, T] ``factor`` times, and
    ``lengths`` [B] int32 = the row sums of ``mask`` times ``factor`` (include/nmhip_split.h), in one launch."""
    bsz, steps = mask.shape
    assert _f32(mask).is_contiguous() and mask.dim() == 2
    assert tuple(_f32(out_mask).shape) == (bsz, steps * int(factor)) and out_mask.is_contiguous()
    assert tuple(_i32(lengths).shape) == (bsz,) and lengths.is_contiguous()
    _lib.check(_lib.load().nm_split_mask(_stream(), mask.data_ptr(), bsz, steps, int(factor), out_mask.data_ptr(),
                                         lengths.data_ptr()), "nm_split_mask")
    return out_mask, lengths


def time_softmax_fwd(e, mask, w, s_out=None, z_out=None):
    """encoders/attentive.py:60-75 on energies [B, T, H], normalised along T: w = softmax_t(e) * mask, renormalised with
    1e-8 in the denominator (mask None: the plain softmax).  ``s_out`` [B, T, H] and ``z_out`` [B, H] are what
    ``time_softmax_bwd`` reads."""
    bsz, steps, h, lde = _btd(e, "time_softmax_fwd e")
    assert tuple(w.shape) == (bsz, steps, h)
    ldw = _btd(w, "time_softmax_fwd w")[3]
    lds = 0
    if s_out is not None:
        assert tuple(s_out.shape) == (bsz, steps, h)
        lds = _btd(s_out, "time_softmax_fwd s_out")[3]
    if mask is not None:
        assert tuple(mask.shape) == (bsz, steps) and _f32(mask).is_contiguous()
    if z_out is not None:
        assert tuple(_f32(z_out).shape) == (bsz, h) and z_out.is_contiguous()
    _lib.check(_lib.load().nm_time_softmax_fwd(_stream(), e.data_ptr(), lde, _p(mask), bsz, steps, h, w.data_ptr(), ldw,
                                               _p(s_out), lds, _p(z_out)), "nm_time_softmax_fwd")
    return w


def time_softmax_bwd(dw, s, z, mask, de, accumulate=False):
    """de (+)= the gradient of ``time_softmax_fwd`` from dw, with s and Z of the forward call."""
    bsz, steps, h, lddw = _btd(dw, "time_softmax_bwd dw")
    assert tuple(s.shape) == (bsz, steps, h) and tuple(de.shape) == (bsz, steps, h)
    lds = _btd(s, "time_softmax_bwd s")[3]
    ldde = _btd(de, "time_softmax_bwd de")[3]
    if mask is not None:
        assert tuple(mask.shape) == (bsz, steps) and _f32(mask).is_contiguous()
        assert tuple(_f32(z).shape) == (bsz, h) and z.is_contiguous()
    _lib.check(_lib.load().nm_time_softmax_bwd(_stream(), dw.data_ptr(), lddw, s.data_ptr(), lds, _p(z), _p(mask), bsz,
                                               steps, h, de.data_ptr(), ldde, int(bool(accumulate))),
               "nm_time_softmax_bwd")
    return de


def sqerr_rows(pred, targets, grad_scale=None, write_grad=False, loss_rows=None):
    """decoders/sequence_regressor.py:76-79 per row: ``loss_rows`` [R] = sum_k (pred[r, k] - targets[r])^2; with
    ``write_grad`` the predictions [R, dim] become grad_scale[0] * 2 (pred - targets) in place."""
    _f32(pred)
    assert pred.dim() == 2
    rows, dim = pred.shape
    ld = _ld2(pred, dim, "sqerr_rows pred")
    assert _f32(targets).numel() == rows and targets.is_contiguous()
    assert loss_rows is None or (_f32(loss_rows).numel() == rows and loss_rows.is_contiguous())
    _lib.check(_lib.load().nm_sqerr_rows(_stream(), pred.data_ptr(), ld, rows, dim, targets.data_ptr(), _p(grad_scale),
                                         int(bool(write_grad)), _p(loss_rows)), "nm_sqerr_rows")
    return loss_rows


# ---- the image stack (include/nmhip_image.h, csrc/nm_image.hip) ------------------------------------------------------------
PADDINGS = {"valid": 0, "same": 1}
WINDOW_MODES = {"max": 0, "avg": 1}
BN_EPSILON = 1e-3           # tf.layers.batch_normalization's defaults (encoders/cnn_encoder.py:107)
BN_MOMENTUM = 0.99


def _nhwc(x, what):
    """(B, H, W, C, row stride) of an NHWC map whose (b, y, x) rows lie one row stride apart."""
    _f32(x)
    assert x.dim() == 4, what
    bsz, h, w, c = x.shape
    assert c == 1 or x.stride(3) == 1, what + ": unit channel stride"
    ld = x.stride(2) if w > 1 else max(x.stride(2), c)
    assert (h == 1 or x.stride(1) == w * ld) and (bsz == 1 or x.stride(0) == h * w * ld), what + ": rows one stride apart"
    return bsz, h, w, c, ld


def conv2d_out_hw(h, w, k, padding):
    """Height and width of a stride-1 convolution's output."""
    return (h, w) if padding == "same" else (h - k + 1, w - k + 1)


def window2d_out_hw(h, w, window, stride, padding):
    """Height and width of a pooled map (TensorFlow's SAME / VALID arithmetic)."""
    if padding == "same":
        return -(-h // stride[0]), -(-w // stride[1])
    return (h - window[0]) // stride[0] + 1, (w - window[1]) // stride[1] + 1


def conv2d_workspace_floats(bsz, h, w, cin, k, cout, padding) -> int:
    """Floats of the workspace ``conv2d_bwd`` needs for the filter and bias gradients of this shape."""
    return int(_lib.load().nm_conv2d_workspace_bytes(bsz, h, w, cin, k, cout, PADDINGS[padding])) // 4


def conv2d_fwd(x, filt, bias, y, padding, algo=0):
    """y [B, OH, OW, Cout] = conv2d(x [B, H, W, Cin], filt [k, k, Cin, Cout]) + bias at stride 1 (nm_conv2d_fwd)."""
    bsz, h, w, cin, ldx = _nhwc(x, "conv2d_fwd x")
    _f32(filt), _f32(bias)
    assert filt.dim() == 4 and filt.is_contiguous() and filt.shape[0] == filt.shape[1] and filt.shape[2] == cin, "filter"
    k, cout = int(filt.shape[0]), int(filt.shape[3])
    assert bias.is_contiguous() and bias.numel() == cout
    oh, ow = conv2d_out_hw(h, w, k, padding)
    assert tuple(y.shape) == (bsz, oh, ow, cout), (tuple(y.shape), (bsz, oh, ow, cout))
    ldy = _nhwc(y, "conv2d_fwd y")[4]
    _lib.check(_lib.load().nm_conv2d_fwd(_stream(), x.data_ptr(), ldx, bsz, h, w, cin, filt.data_ptr(), k, cout,
                                         PADDINGS[padding], bias.data_ptr(), y.data_ptr(), ldy, int(algo)), "nm_conv2d_fwd")
    return y


def conv2d_bwd(x, filt, dy, padding, dx=None, accumulate_dx=False, dfilt=None, dbias=None, accumulate_params=True,
               workspace=None, algo=0):
    """The gradient of ``conv2d_fwd``: dx (+)= conv2d^T(dy, filt); dfilt / dbias (+)= the filter / bias gradients
    (nm_conv2d_bwd; deterministic).  ``workspace``: conv2d_workspace_floats floats, needed with ``dfilt`` / ``dbias``."""
    bsz, h, w, cin, ldx = _nhwc(x, "conv2d_bwd x")
    _f32(filt)
    assert filt.dim() == 4 and filt.is_contiguous() and filt.shape[0] == filt.shape[1] and filt.shape[2] == cin, "filter"
    k, cout = int(filt.shape[0]), int(filt.shape[3])
    oh, ow = conv2d_out_hw(h, w, k, padding)
    assert tuple(dy.shape) == (bsz, oh, ow, cout)
    lddy = _nhwc(dy, "conv2d_bwd dy")[4]
    lddx = 0
    if dx is not None:
        assert tuple(dx.shape) == (bsz, h, w, cin)
        lddx = _nhwc(dx, "conv2d_bwd dx")[4]
    assert dfilt is None or (_f32(dfilt).is_contiguous() and dfilt.numel() == filt.numel())
    assert dbias is None or (_f32(dbias).is_contiguous() and dbias.numel() == cout)
    _lib.check(_lib.load().nm_conv2d_bwd(_stream(), x.data_ptr(), ldx, bsz, h, w, cin, filt.data_ptr(), k, cout,
                                         PADDINGS[padding], dy.data_ptr(), lddy, _p(dx), lddx, int(bool(accumulate_dx)),
                                         _p(dfilt), _p(dbias), int(bool(accumulate_params)), _p(workspace),
                                         0 if workspace is None else workspace.numel() * 4, int(algo)), "nm_conv2d_bwd")


def bn2d_fwd(x, gamma, beta, y, training, relu, moving_mean=None, moving_var=None, batch_mean=None, batch_var=None,
             eps=BN_EPSILON, momentum=BN_MOMENTUM):
    """Batch normalisation over the rows of x [rows, C] (+ ReLU) (nm_bn2d_fwd): training mode writes ``batch_mean`` /
    ``batch_var`` and, when given, updates the moving statistics; inference reads the moving statistics."""
    c = x.shape[1]
    ldx, ldy = _ld2(x, c, "bn2d_fwd x"), _ld2(y, c, "bn2d_fwd y")
    assert y.shape == x.shape
    for t in (gamma, beta, moving_mean, moving_var, batch_mean, batch_var):
        assert t is None or (_f32(t).is_contiguous() and t.numel() == c)
    _lib.check(_lib.load().nm_bn2d_fwd(_stream(), x.data_ptr(), ldx, x.shape[0], c, gamma.data_ptr(), beta.data_ptr(),
                                       float(eps), float(momentum), int(bool(training)), int(bool(relu)),
                                       _p(moving_mean), _p(moving_var), _p(batch_mean), _p(batch_var), y.data_ptr(), ldy),
               "nm_bn2d_fwd")
    return y


def bn2d_bwd(x, y, dy, gamma, batch_mean, batch_var, relu, sums, dx=None, accumulate_dx=False, dgamma=None, dbeta=None,
             accumulate_params=True, eps=BN_EPSILON):
    """The gradient of the training-mode ``bn2d_fwd`` (nm_bn2d_bwd); ``sums`` [2C] is scratch."""
    c = x.shape[1]
    ldx, lddy = _ld2(x, c, "bn2d_bwd x"), _ld2(dy, c, "bn2d_bwd dy")
    ldy = 0 if y is None else _ld2(y, c, "bn2d_bwd y")
    lddx = 0 if dx is None else _ld2(dx, c, "bn2d_bwd dx")
    assert dy.shape == x.shape and (dx is None or dx.shape == x.shape) and (y is None or y.shape == x.shape)
    assert _f32(sums).is_contiguous() and sums.numel() == 2 * c
    for t in (gamma, batch_mean, batch_var, dgamma, dbeta):
        assert t is None or (_f32(t).is_contiguous() and t.numel() == c)
    _lib.check(_lib.load().nm_bn2d_bwd(_stream(), x.data_ptr(), ldx, _p(y), ldy, dy.data_ptr(), lddy, x.shape[0], c,
                                       gamma.data_ptr(), batch_mean.data_ptr(), batch_var.data_ptr(), float(eps),
                                       int(bool(relu)), _p(dx), lddx, int(bool(accumulate_dx)), _p(dgamma), _p(dbeta),
                                       int(bool(accumulate_params)), sums.data_ptr()), "nm_bn2d_bwd")


# the same batch norm with statistics over the rows of all ranks (include/nmhip_bnsync.h, csrc/nm_bnsync.hip)
def bn2d_part_doubles(c) -> int:
    """Doubles of one rank's part: the row count, C means, C sums of squared deviations."""
    return 2 * int(c) + 1


def _f64(t):
    assert t.dtype == torch.float64 and t.is_cuda, (t.dtype, t.device)
    return t


def bn2d_part_stats(x, part):
    """This rank's part of the statistics of x [rows, C] into ``part`` (float64 [2C + 1]) (nm_bn2d_part_stats)."""
    c = x.shape[1]
    ldx = _ld2(x, c, "bn2d_part_stats x")
    assert _f64(part).is_contiguous() and part.numel() == bn2d_part_doubles(c)
    _lib.check(_lib.load().nm_bn2d_part_stats(_stream(), x.data_ptr(), ldx, x.shape[0], c, part.data_ptr()),
               "nm_bn2d_part_stats")
    return part


def bn2d_merge(parts, batch_mean, batch_var, total, moving_mean=None, moving_var=None, momentum=BN_MOMENTUM):
    """The statistics of all rows from ``parts`` (float64 [world, 2C + 1], in rank order) (nm_bn2d_merge): the mean, the
    biased variance, ``total`` (float64 [1]: the row count) and, when given, the moving statistics' step."""
    c = batch_mean.numel()
    assert _f64(parts).is_contiguous() and parts.dim() == 2 and parts.shape[1] == bn2d_part_doubles(c)
    assert _f64(total).numel() == 1
    for t in (moving_mean, moving_var, batch_mean, batch_var):
        assert t is None or (_f32(t).is_contiguous() and t.numel() == c)
    _lib.check(_lib.load().nm_bn2d_merge(_stream(), parts.data_ptr(), parts.shape[0], c, float(momentum), _p(moving_mean),
                                         _p(moving_var), batch_mean.data_ptr(), batch_var.data_ptr(), total.data_ptr()),
               "nm_bn2d_merge")


def bn2d_bwd_sums(x, y, dy, mean, var, relu, sums, dgamma=None, dbeta=None, accumulate_params=True, eps=BN_EPSILON):
    """The first half of ``bn2d_bwd`` from the merged ``mean`` / ``var``: this rank's two channel sums into ``sums``
    [2C], and into ``dgamma`` / ``dbeta`` (nm_bn2d_bwd_sums)."""
    c = x.shape[1]
    ldx, lddy = _ld2(x, c, "bn2d_bwd_sums x"), _ld2(dy, c, "bn2d_bwd_sums dy")
    ldy = 0 if y is None else _ld2(y, c, "bn2d_bwd_sums y")
    assert dy.shape == x.shape and (y is None or y.shape == x.shape)
    assert _f32(sums).is_contiguous() and sums.numel() == 2 * c
    for t in (mean, var, dgamma, dbeta):
        assert t is None or (_f32(t).is_contiguous() and t.numel() == c)
    _lib.check(_lib.load().nm_bn2d_bwd_sums(_stream(), x.data_ptr(), ldx, _p(y), ldy, dy.data_ptr(), lddy, x.shape[0], c,
                                            mean.data_ptr(), var.data_ptr(), float(eps), int(bool(relu)),
                                            sums.data_ptr(), _p(dgamma), _p(dbeta), int(bool(accumulate_params))),
               "nm_bn2d_bwd_sums")


def bn2d_bwd_dx(x, y, dy, gamma, mean, var, relu, sums, n, dx, accumulate_dx=False, eps=BN_EPSILON):
    """The second half: dx from ``sums`` [2C] added over all ranks and the global row count ``n`` (nm_bn2d_bwd_dx)."""
    c = x.shape[1]
    ldx, lddy, lddx = _ld2(x, c, "bn2d_bwd_dx x"), _ld2(dy, c, "bn2d_bwd_dx dy"), _ld2(dx, c, "bn2d_bwd_dx dx")
    ldy = 0 if y is None else _ld2(y, c, "bn2d_bwd_dx y")
    assert dy.shape == x.shape and dx.shape == x.shape and (y is None or y.shape == x.shape)
    assert _f32(sums).is_contiguous() and sums.numel() == 2 * c
    for t in (gamma, mean, var):
        assert _f32(t).is_contiguous() and t.numel() == c
    _lib.check(_lib.load().nm_bn2d_bwd_dx(_stream(), x.data_ptr(), ldx, _p(y), ldy, dy.data_ptr(), lddy, x.shape[0], c,
                                          gamma.data_ptr(), mean.data_ptr(), var.data_ptr(), float(eps),
                                          int(bool(relu)), sums.data_ptr(), int(n), dx.data_ptr(), lddx,
                                          int(bool(accumulate_dx))), "nm_bn2d_bwd_dx")


def window2d_fwd(mode, x, y, window, stride, padding="valid", argmax=None):
    """y [B, OH, OW, C] = max / average of x [B, H, W, C] over ``window`` at ``stride`` (nm_window2d_fwd); ``argmax``
    (int32, the shape of y, contiguous): where the first maximum lies, for ``window2d_bwd``."""
    bsz, h, w, c, ldx = _nhwc(x, "window2d_fwd x")
    oh, ow = window2d_out_hw(h, w, window, stride, padding)
    assert tuple(y.shape) == (bsz, oh, ow, c), (tuple(y.shape), (bsz, oh, ow, c))
    ldy = _nhwc(y, "window2d_fwd y")[4]
    assert argmax is None or (_i32(argmax).is_contiguous() and argmax.numel() == y.numel())
    _lib.check(_lib.load().nm_window2d_fwd(_stream(), x.data_ptr(), ldx, bsz, h, w, c, window[0], window[1], stride[0],
                                           stride[1], PADDINGS[padding], WINDOW_MODES[mode], y.data_ptr(), ldy,
                                           _p(argmax)), "nm_window2d_fwd")
    return y


def window2d_bwd(mode, dy, dx, window, stride, padding="valid", argmax=None, accumulate=False):
    """dx [B, H, W, C] (+)= the gradient of ``window2d_fwd`` (nm_window2d_bwd); every element is written."""
    bsz, h, w, c, lddx = _nhwc(dx, "window2d_bwd dx")
    oh, ow = window2d_out_hw(h, w, window, stride, padding)
    assert tuple(dy.shape) == (bsz, oh, ow, c)
    lddy = _nhwc(dy, "window2d_bwd dy")[4]
    assert argmax is None or (_i32(argmax).is_contiguous() and argmax.numel() == dy.numel())
    _lib.check(_lib.load().nm_window2d_bwd(_stream(), dy.data_ptr(), lddy, _p(argmax), bsz, h, w, c, window[0], window[1],
                                           stride[0], stride[1], PADDINGS[padding], WINDOW_MODES[mode], dx.data_ptr(),
                                           lddx, int(bool(accumulate))), "nm_window2d_bwd")
    return dx


def map_columns(src, dst, inverse=False):
    """dst [B, W, H*C] = the columns of the map src [B, H, W, C], left to right (nm_map_columns); ``inverse``: the map
    dst [B, H, W, C] from its columns src [B, W, H*C]."""
    bsz, h, w, c = (dst if inverse else src).shape
    cols = src if inverse else dst
    assert tuple(cols.shape) == (bsz, w, h * c) and _f32(src).is_contiguous() and _f32(dst).is_contiguous()
    _lib.check(_lib.load().nm_map_columns(_stream(), src.data_ptr(), dst.data_ptr(), bsz, h, w, c, int(bool(inverse))),
               "nm_map_columns")
    return dst


# ---- the frozen ImageNet networks (include/nmhip_vgg.h, csrc/nm_vgg.hip) ----------------------------------------------------
CONV_ACT_TILES = {None: 0, "auto": 0, "128x64": 1, "64x64": 2}


def conv2d_act_fwd(x, filt, bias, y, padding, relu=True, tile=None):
    """y [B, OH, OW, Cout] = act(conv2d(x [B, H, W, Cin], filt [k, k, Cin, Cout]) + bias) at stride 1, forward only
    (nm_conv2d_act_fwd): act is the ReLU or, with ``relu=False``, nothing; ``bias`` may be None."""
    bsz, h, w, cin, ldx = _nhwc(x, "conv2d_act_fwd x")
    _f32(filt)
    assert filt.dim() == 4 and filt.is_contiguous() and filt.shape[0] == filt.shape[1] and filt.shape[2] == cin, "filter"
    k, cout = int(filt.shape[0]), int(filt.shape[3])
    assert bias is None or (_f32(bias).is_contiguous() and bias.numel() == cout)
    oh, ow = conv2d_out_hw(h, w, k, padding)
    assert tuple(y.shape) == (bsz, oh, ow, cout), (tuple(y.shape), (bsz, oh, ow, cout))
    ldy = _nhwc(y, "conv2d_act_fwd y")[4]
    _lib.check(_lib.load().nm_conv2d_act_fwd(_stream(), x.data_ptr(), ldx, bsz, h, w, cin, filt.data_ptr(), k, cout,
                                             PADDINGS[padding], _p(bias), int(bool(relu)), y.data_ptr(), ldy,
                                             CONV_ACT_TILES[tile]), "nm_conv2d_act_fwd")
    return y


# ---- rewards of self-critical training (include/nmhip_reward.h, csrc/nm_reward.hip) ----------------------------------------
REWARD_KINDS = {"bleu": 0, "gleu": 1}


def sentence_reward_max_tokens() -> int:
    return int(_lib.load().nm_sentence_reward_max_tokens())


def sentence_reward(kind, references, hypotheses, end_id, out=None):
    """Sentence-level BLEU (``kind`` "bleu") or GLEU ("gleu") on token indices, one float per sentence
    (trainers/self_critical_objective.py:124-231): ``references`` [T_ref, B] and ``hypotheses`` [T_hyp, B] are int32,
    time-major, with unit batch stride and any row stride."""
    lib = _lib.load()
    _i32(references), _i32(hypotheses)
    assert references.dim() == 2 and hypotheses.dim() == 2 and references.shape[1] == hypotheses.shape[1]
    bsz = references.shape[1]
    strides = []
    for t in (references, hypotheses):
        assert bsz == 1 or t.stride(1) == 1, "unit batch stride"
        strides.append(t.stride(0) if t.shape[0] > 1 else max(t.stride(0), bsz))
    if out is None:
        out = torch.empty(bsz, dtype=torch.float32, device=references.device)
    assert _f32(out).numel() == bsz and out.is_contiguous()
    _lib.check(lib.nm_sentence_reward(_stream(), REWARD_KINDS[kind], references.data_ptr(), strides[0],
                                      references.shape[0], hypotheses.data_ptr(), strides[1], hypotheses.shape[0], bsz,
                                      int(end_id), out.data_ptr()), "nm_sentence_reward")
    return out


def reinforce_weights(reward, baseline, mask, weight, weights, grad_scale, inv_count):
    """``weights`` [T, B] = -(reward - baseline)[None, :] * mask, ``grad_scale`` [1] = weight / sum(mask) and
    ``inv_count`` [1] = 1 / sum(mask) from the int32 runtime ``mask`` [T, B], all on the device
    (trainers/self_critical_objective.py:75-85,113-120): the operands of ``xent`` over the runtime logits."""
    lib = _lib.load()
    assert _i32(mask).dim() == 2 and mask.is_contiguous()
    steps, bsz = mask.shape
    for t, n in ((reward, bsz), (baseline, bsz), (weights, steps * bsz), (grad_scale, 1), (inv_count, 1)):
        assert _f32(t).numel() == n and t.is_contiguous()
    _lib.check(lib.nm_reinforce_weights(_stream(), reward.data_ptr(), baseline.data_ptr(), mask.data_ptr(), steps, bsz,
                                        float(weight), weights.data_ptr(), grad_scale.data_ptr(), inv_count.data_ptr()),
               "nm_reinforce_weights")
    return weights


# ---- minimum Bayes risk decoding over samples (include/nmhip_mbr.h, csrc/nm_mbr.hip) ------------------------------------------
def _mbr_samples(token_ids):
    """(row stride, T, B, n) of the samples [T, B, n] int32: sample j of sentence b at ``b * n + j`` of a row."""
    assert _i32(token_ids).dim() == 3, tuple(token_ids.shape)
    steps, bsz, n = token_ids.shape
    assert n == 1 or token_ids.stride(2) == 1, "unit sample stride"
    assert bsz == 1 or token_ids.stride(1) == n, "the samples of a sentence side by side"
    return (token_ids.stride(0) if steps > 1 else max(token_ids.stride(0), bsz * n)), steps, bsz, n


def mbr_pairwise(kind, token_ids, end_id, out=None):
    """``out`` [B, n, n] float32: the sentence-level BLEU (``kind`` "bleu") or GLEU ("gleu") of every ordered pair of
    the ``n`` samples of a sentence, ``out[b, i, j]`` with sample ``j`` as the reference and sample ``i`` as the
    hypothesis.  ``token_ids`` [T, B, n] int32 as ``SamplingOutput.token_ids`` (any row stride)."""
    stride, steps, bsz, n = _mbr_samples(token_ids)
    if out is None:
        out = torch.empty((bsz, n, n), dtype=torch.float32, device=token_ids.device)
    assert tuple(_f32(out).shape) == (bsz, n, n) and out.is_contiguous()
    _lib.check(_lib.load().nm_mbr_pairwise(_stream(), REWARD_KINDS[kind], token_ids.data_ptr(), stride, steps, bsz, n,
                                           int(end_id), out.data_ptr()), "nm_mbr_pairwise")
    return out


def mbr_select(utilities, token_ids, expected=None, best=None, chosen=None):
    """(``expected`` [B, n] float32, ``best`` [B] int32, ``chosen`` [T, B] int32) from ``utilities`` [B, n, n] of any
    origin: the mean of every row (summed in double, in index order), the row with the largest sum (ties to the lowest
    index, NaN last) and that sample's column of ``token_ids`` [T, B, n]."""
    stride, steps, bsz, n = _mbr_samples(token_ids)
    assert tuple(_f32(utilities).shape) == (bsz, n, n) and utilities.is_contiguous()
    dev = token_ids.device
    expected = torch.empty((bsz, n), dtype=torch.float32, device=dev) if expected is None else expected
    best = torch.empty((bsz,), dtype=torch.int32, device=dev) if best is None else best
    chosen = torch.empty((steps, bsz), dtype=torch.int32, device=dev) if chosen is None else chosen
    assert tuple(_f32(expected).shape) == (bsz, n) and expected.is_contiguous()
    assert tuple(_i32(best).shape) == (bsz,) and best.is_contiguous()
    assert tuple(_i32(chosen).shape) == (steps, bsz) and chosen.is_contiguous()
    _lib.check(_lib.load().nm_mbr_select(_stream(), utilities.data_ptr(), token_ids.data_ptr(), stride, steps, bsz, n,
                                         expected.data_ptr(), best.data_ptr(), chosen.data_ptr()), "nm_mbr_select")
    return expected, best, chosen


# ---- REINFORCE with sentence-level feedback (include/nmhip_rl.h, csrc/nm_rl.hip) --------------------------------------------
def eval_sentence_score_max_tokens() -> int:
    return int(_lib.load().nm_eval_sentence_score_max_tokens())


def eval_sentence_score(kind, order, references, hypotheses, end_id, pad_id, out=None):
    """The evaluators' sentence BLEU (``kind`` "bleu", times 100) or GLEU ("gleu") over the 1- to ``order``-grams as
    trainers/rl_trainer.py:83-115 scores a sample, on token indices, one float per sentence: ``references`` [T_ref, B]
    and ``hypotheses`` [T_hyp, B] are int32, time-major, with unit batch stride and any row stride, each cut at its
    first ``end_id`` or ``pad_id``."""
    lib = _lib.load()
    _i32(references), _i32(hypotheses)
    assert references.dim() == 2 and hypotheses.dim() == 2 and references.shape[1] == hypotheses.shape[1]
    bsz = references.shape[1]
    strides = []
    for t in (references, hypotheses):
        assert bsz == 1 or t.stride(1) == 1, "unit batch stride"
        strides.append(t.stride(0) if t.shape[0] > 1 else max(t.stride(0), bsz))
    if out is None:
        out = torch.empty(bsz, dtype=torch.float32, device=references.device)
    assert _f32(out).numel() == bsz and out.is_contiguous()
    _lib.check(lib.nm_eval_sentence_score(_stream(), REWARD_KINDS[kind], int(order), references.data_ptr(), strides[0],
                                          references.shape[0], hypotheses.data_ptr(), strides[1], hypotheses.shape[0],
                                          bsz, int(end_id), int(pad_id), out.data_ptr()), "nm_eval_sentence_score")
    return out


# ---- ... over a vocabulary of subword pieces (include/nmhip_subword.h, csrc/nm_subword.hip) ----------------------------------
PIECE_TABLE_ROW = 12


def eval_joined_sentence_score_max_tokens() -> int:
    return int(_lib.load().nm_eval_joined_sentence_score_max_tokens())


def eval_joined_sentence_score(kind, order, references, hypotheses, table, out=None):
    """``eval_sentence_score`` over the indices of subword PIECES: the words compared are those of the reference's join
    (trainers/rl_trainer.py:110-111), each identified by its length in bytes and two polynomial hashes composed from
    the rows of ``table`` -- int32 [V, 12] on the device, ``trainers.rl_trainer.piece_table`` of the vocabulary.
    ``references`` [T_ref, B] and ``hypotheses`` [T_hyp, B] are int32, time-major, with unit batch stride and any row
    stride, each cut at its first token the table flags as ``</s>`` or ``<pad>`` (or whose id is outside the table)."""
    lib = _lib.load()
    _i32(references), _i32(hypotheses), _i32(table)
    assert references.dim() == 2 and hypotheses.dim() == 2 and references.shape[1] == hypotheses.shape[1]
    assert table.dim() == 2 and table.shape[1] == PIECE_TABLE_ROW and table.is_contiguous()
    assert table.device == references.device == hypotheses.device
    bsz = references.shape[1]
    strides = []
    for t in (references, hypotheses):
        assert bsz == 1 or t.stride(1) == 1, "unit batch stride"
        strides.append(t.stride(0) if t.shape[0] > 1 else max(t.stride(0), bsz))
    if out is None:
        out = torch.empty(bsz, dtype=torch.float32, device=references.device)
    assert _f32(out).numel() == bsz and out.is_contiguous()
    _lib.check(lib.nm_eval_joined_sentence_score(_stream(), REWARD_KINDS[kind], int(order), references.data_ptr(),
                                                 strides[0], references.shape[0], hypotheses.data_ptr(), strides[1],
                                                 hypotheses.shape[0], bsz, table.data_ptr(), table.shape[0],
                                                 table.shape[0], out.data_ptr()), "nm_eval_joined_sentence_score")
    return out


def reinforce_sample_weights(rewards, sent_logprobs, steps, weights, grad_scale, loss, baseline, weight=1.0,
                             subtract_baseline=False, normalize=False, alpha=1.0, reward_counter=None, reward_sum=None):
    """trainers/rl_trainer.py:149-185 in one launch: from ``rewards`` and ``sent_logprobs`` [S, B], the host list
    ``steps`` of the S loop lengths and the baseline's two device scalars (updated in place) to the row weights
    ``weights`` [S, T, B] of ``xent`` over each sample's logits, ``grad_scale`` [1] = ``weight``, ``loss`` [1] and
    ``baseline`` [1]."""
    import ctypes
    lib = _lib.load()
    samples, tmax, bsz = weights.shape
    assert weights.is_contiguous() and _f32(weights) is not None and len(steps) == samples
    for t, n in ((rewards, samples * bsz), (sent_logprobs, samples * bsz), (grad_scale, 1), (loss, 1), (baseline, 1),
                 (reward_counter, 1), (reward_sum, 1)):
        assert t is None or (_f32(t).numel() == n and t.is_contiguous())
    host_steps = (ctypes.c_int32 * samples)(*[int(n) for n in steps])
    _lib.check(lib.nm_reinforce_sample_weights(_stream(), rewards.data_ptr(), _p(sent_logprobs), host_steps, samples,
                                               tmax, bsz, int(bool(subtract_baseline)), int(bool(normalize)),
                                               float(alpha), float(weight), _p(reward_counter), _p(reward_sum),
                                               weights.data_ptr(), grad_scale.data_ptr(), _p(loss),
                                               baseline.data_ptr()), "nm_reinforce_sample_weights")
    return weights


def reinforce_sample_weights_max_samples() -> int:
    return int(_lib.load().nm_reinforce_sample_weights_max_samples())
