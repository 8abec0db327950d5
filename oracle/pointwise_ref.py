"""Plain restatements of the point-wise, sequence-utility and backward operations of the general (taped) path --
what include/nmhip.h documents for nm_ew, the fused cells, nm_blend_*, nm_rnn_select_*, nm_reverse_sequence,
nm_maxout_*, nm_dropout, nm_embedding_scatter_add, nm_layer_norm_bwd, nm_attn_softmax_*, the Transformer utilities,
nm_reduce_sum, nm_log_softmax, nm_greedy_update and nm_gemm_f32_group.

Every function computes in the dtype of its inputs: the GPU tests evaluate it in float64, the CPU tests evaluate it in
float32 as well to show that a test's bound can be met by plain fp32 arithmetic on the same inputs.

Forward operations are written from the formulas of the header (and the reference call sites it cites); backward
operations are ``torch.autograd`` of the forward restatement -- no derivative is written out by hand here, so a mistake
in a kernel's own derivation cannot be shared."""
from typing import Optional, Sequence

import numpy as np
import torch

from oracle.general_ref import dropout_mask

EW_OPS = ("copy", "add", "sub", "mul", "scale", "sigmoid", "tanh", "relu", "sigmoid_bwd", "tanh_bwd", "relu_bwd",
          "logaddexp", "add_scalar", "rowscale", "div")
EW_BINARY = ("add", "sub", "mul", "sigmoid_bwd", "tanh_bwd", "relu_bwd", "logaddexp", "rowscale", "div")
# single correctly-rounded fp32 operations (or copies / selects): compared bit for bit
EW_EXACT = ("add", "sub", "mul", "div", "scale", "add_scalar", "copy", "relu", "relu_bwd", "rowscale")


def _t(x, dtype=None):
    """torch view of a NumPy array (or tensor), optionally converted."""
    t = torch.as_tensor(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    return t if dtype is None else t.to(dtype)


def _sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


# --------------------------------------------------------------------------------------------------------------
# nm_ew: the op codes of include/nmhip.h
# --------------------------------------------------------------------------------------------------------------
def ew(op: str, a: np.ndarray, b: Optional[np.ndarray] = None, alpha: float = 0.0) -> np.ndarray:
    """f(a, b) of one nm_ew op code, in the dtype of ``a`` (``alpha`` is rounded to it)."""
    dt = a.dtype.type
    al = dt(alpha)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if op == "copy":
            return a.copy()
        if op == "add":
            return a + b
        if op == "sub":
            return a - b
        if op == "mul":
            return a * b
        if op == "scale":
            return al * a
        if op == "sigmoid":
            return dt(1.0) / (dt(1.0) + np.exp(-(a + al)))
        if op == "tanh":
            return np.tanh(a)
        if op == "relu":
            return np.maximum(a, dt(0.0))
        if op == "sigmoid_bwd":          # a = the forward output, b = the upstream gradient
            return b * a * (dt(1.0) - a)
        if op == "tanh_bwd":
            return b * (dt(1.0) - a * a)
        if op == "relu_bwd":
            return np.where(a > 0, b, dt(0.0)).astype(a.dtype)
        if op == "logaddexp":            # log(exp(a) + exp(b)); -inf on both sides is -inf
            return np.logaddexp(a, b)
        if op == "add_scalar":
            return a + al
        if op == "rowscale":             # b [rows, 1]
            return a * b.reshape(-1, 1)
        if op == "div":
            return a / b
    raise ValueError(op)


# --------------------------------------------------------------------------------------------------------------
# LSTMCell (tf.nn.rnn_cell.LSTMCell: gate order i, j, f, o; forget_bias added to f)
# --------------------------------------------------------------------------------------------------------------
def lstm_cell(z, c_prev, forget_bias: float):
    """z [R, 4H] = [i | j | f | o] pre-activations -> (c_new, h_new, activated gates [R, 4H])."""
    z, c_prev = _t(z), _t(c_prev)
    i, j, f, o = torch.chunk(z, 4, dim=1)
    gi, gj, gf, go = _sigmoid(i), torch.tanh(j), _sigmoid(f + forget_bias), _sigmoid(o)
    c_new = gf * c_prev + gi * gj
    h_new = go * torch.tanh(c_new)
    return c_new, h_new, torch.cat([gi, gj, gf, go], dim=1)


def lstm_cell_grads(z, c_prev, forget_bias: float, dh=None, dc_new=None):
    """(dz, dc_prev) by autograd of ``lstm_cell`` for upstream gradients dh / dc_new (None: no gradient from there)."""
    z = _t(z).clone().requires_grad_(True)
    c_prev = _t(c_prev).clone().requires_grad_(True)
    c_new, h_new, _ = lstm_cell(z, c_prev, forget_bias)
    loss = z.sum() * 0.0
    if dh is not None:
        loss = loss + (h_new * _t(dh)).sum()
    if dc_new is not None:
        loss = loss + (c_new * _t(dc_new)).sum()
    dz, dc_prev = torch.autograd.grad(loss, [z, c_prev])
    return dz, dc_prev


# --------------------------------------------------------------------------------------------------------------
# NematusGRUCell (nn/ortho_gru_cell.py:73-105): the reset gate multiplies the state projection after the product
# --------------------------------------------------------------------------------------------------------------
def nematus_cell(g_pre, sc, ci, h_prev, g2=None):
    """-> (h_new, ru [R, 2H] = [r | u], c)."""
    g_pre, sc, ci, h_prev = _t(g_pre), _t(sc), _t(ci), _t(h_prev)
    if g2 is not None:
        g_pre = g_pre + _t(g2)
    ru = _sigmoid(g_pre)
    r, u = torch.chunk(ru, 2, dim=1)
    c = torch.tanh(ci + sc * r)
    return u * h_prev + (1.0 - u) * c, ru, c


def nematus_cell_grads(g_pre, sc, ci, h_prev, dh, g2=None):
    """(dg, dci, dsc, dh_prev) by autograd; the gradient of ``g2`` equals dg (it enters through the same sum)."""
    leaves = [_t(x).clone().requires_grad_(True) for x in (g_pre, ci, sc, h_prev)]
    h_new, _, _ = nematus_cell(leaves[0], leaves[2], leaves[1], leaves[3], g2)
    return torch.autograd.grad((h_new * _t(dh)).sum(), leaves)


# --------------------------------------------------------------------------------------------------------------
# h' = u h + (1 - u) c
# --------------------------------------------------------------------------------------------------------------
def blend(u, h, c):
    u, h, c = _t(u), _t(h), _t(c)
    return u * h + (1.0 - u) * c


def blend_grads(dy, u, h, c):
    leaves = [_t(x).clone().requires_grad_(True) for x in (u, h, c)]
    return torch.autograd.grad((blend(*leaves) * _t(dy)).sum(), leaves)


# --------------------------------------------------------------------------------------------------------------
# dynamic_rnn(sequence_length) step t: rows with t >= lengths[r] carry h_prev through and emit zeros
# --------------------------------------------------------------------------------------------------------------
def _live(lengths, t, rows):
    if lengths is None:
        return torch.ones(rows, 1, dtype=torch.bool)
    return (t < torch.as_tensor(np.asarray(lengths))).reshape(rows, 1)


def rnn_select(h_new, h_prev, lengths, t: int):
    """-> (h_out, y_out)."""
    h_new, h_prev = _t(h_new), _t(h_prev)
    live = _live(lengths, t, h_new.shape[0])
    return torch.where(live, h_new, h_prev), torch.where(live, h_new, torch.zeros_like(h_new))


def rnn_select_grads(h_new, h_prev, lengths, t: int, dh=None, dy=None):
    """(d_new, d_prev) by autograd for upstream gradients of h_out / y_out."""
    leaves = [_t(x).clone().requires_grad_(True) for x in (h_new, h_prev)]
    h_out, y_out = rnn_select(leaves[0], leaves[1], lengths, t)
    loss = (leaves[0].sum() + leaves[1].sum()) * 0.0
    if dh is not None:
        loss = loss + (h_out * _t(dh)).sum()
    if dy is not None:
        loss = loss + (y_out * _t(dy)).sum()
    return torch.autograd.grad(loss, leaves)


# --------------------------------------------------------------------------------------------------------------
# tf.reverse_sequence(x [B, S, D], lengths, seq_axis=1): lengths beyond S are clamped
# --------------------------------------------------------------------------------------------------------------
def reverse_sequence(x: np.ndarray, lengths) -> np.ndarray:
    b, s, _ = x.shape
    ln = np.minimum(np.asarray(lengths, dtype=np.int64), s)[:, None]
    pos = np.arange(s)[None, :]
    src = np.where(pos < ln, ln - 1 - pos, pos)
    return x[np.arange(b)[:, None], src]


# --------------------------------------------------------------------------------------------------------------
# maxout (nn/projection.py:7-35): out[r, g] = max_p x[r, p * groups + g]; the first maximum takes the gradient
# --------------------------------------------------------------------------------------------------------------
def maxout(x, pool: int):
    """-> (out [R, G], argmax [R, G] int32)."""
    x = _t(x)
    rows, cols = x.shape
    x3 = x.reshape(rows, pool, cols // pool)
    best = x3.max(dim=1, keepdim=True).values
    first = (x3 == best).to(torch.int32).argmax(dim=1)          # argmax of a 0/1 tensor: the FIRST maximal member
    return x3.gather(1, first[:, None, :].long()).squeeze(1), first.to(torch.int32)


def maxout_grads(x, pool: int, dy):
    x = _t(x).clone().requires_grad_(True)
    out, _ = maxout(x, pool)
    return torch.autograd.grad((out * _t(dy)).sum(), [x])[0]


# --------------------------------------------------------------------------------------------------------------
# dropout with the counter-based mask of oracle/general_ref.py; ``step`` advances the salt
# --------------------------------------------------------------------------------------------------------------
def effective_salt(salt: int, step: Optional[int]) -> int:
    return int(salt) & 0xFFFFFFFF if step is None else (int(salt) + int(step) * 0x9E3779B9) & 0xFFFFFFFF


def dropout(x: np.ndarray, keep_prob: float, salt: int, step: Optional[int] = None) -> np.ndarray:
    mask = dropout_mask(x.size, keep_prob, effective_salt(salt, step)).reshape(x.shape)
    return x * mask.astype(x.dtype)


# --------------------------------------------------------------------------------------------------------------
# dpre = gradient of tanh at ``pre`` (nm_tanh_bwd is handed y = tanh(pre))
# --------------------------------------------------------------------------------------------------------------
def tanh_grads(pre, dy):
    pre = _t(pre).clone().requires_grad_(True)
    return torch.autograd.grad((torch.tanh(pre) * _t(dy)).sum(), [pre])[0]


# --------------------------------------------------------------------------------------------------------------
# embedding lookup gradient: out[i] = table[ids[i]] * (skip_pad ? ids[i] != 0 : 1); ids outside [0, V) give nothing
# --------------------------------------------------------------------------------------------------------------
def embedding_grads(vocab: int, ids, d, skip_pad: bool):
    d = _t(d)
    ids = torch.as_tensor(np.asarray(ids)).long()
    ok = (ids >= 0) & (ids < vocab)
    table = torch.zeros(vocab, d.shape[1], dtype=d.dtype, requires_grad=True)
    rows = table[ids[ok]]
    if skip_pad:
        rows = rows * (ids[ok] != 0).to(d.dtype)[:, None]
    return torch.autograd.grad((rows * d[ok]).sum(), [table])[0]


# --------------------------------------------------------------------------------------------------------------
# layer norm (tf_utils.py:189-219: biased variance, eps inside the rsqrt)
# --------------------------------------------------------------------------------------------------------------
def layer_norm(x, gamma, beta, eps: float = 1e-6):
    """-> (y, xhat, mean [R], rstd [R])."""
    x, gamma, beta = _t(x), _t(gamma), _t(beta)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    xhat = (x - mu) * rstd
    return xhat * gamma + beta, xhat, mu.squeeze(-1), rstd.squeeze(-1)


def layer_norm_grads(x, gamma, beta, dy, eps: float = 1e-6):
    """(dx, dgamma, dbeta) by autograd."""
    leaves = [_t(v).clone().requires_grad_(True) for v in (x, gamma, beta)]
    y = layer_norm(*leaves, eps)[0]
    return torch.autograd.grad((y * _t(dy)).sum(), leaves)


# --------------------------------------------------------------------------------------------------------------
# masked, renormalised softmax: the arithmetic of oracle/nm_oracle.py::attention_step (feed_forward.py:139-144)
# --------------------------------------------------------------------------------------------------------------
def mask_rows(mask, rows: int, bsz: int, rows_per_key: int = 1):
    """The mask row of every query row: (r / rows_per_key) % B."""
    if mask is None:
        return None
    idx = (np.arange(rows) // rows_per_key) % bsz
    return _t(mask)[torch.as_tensor(idx)]


def attn_softmax(e, mask_per_row):
    """w = softmax(e) * m / (sum(softmax(e) * m) + 1e-8); ``mask_per_row`` [rows, S] or None (no mask)."""
    e = _t(e)
    p = torch.softmax(e, dim=-1)
    if mask_per_row is None:
        mask_per_row = torch.ones_like(p)
    w_all = p * mask_per_row.to(e.dtype)
    return w_all / (w_all.sum(-1, keepdim=True) + 1e-8)


def attn_softmax_grads(e, mask_per_row, dw):
    e = _t(e).clone().requires_grad_(True)
    return torch.autograd.grad((attn_softmax(e, mask_per_row) * _t(dw)).sum(), [e])[0]


# --------------------------------------------------------------------------------------------------------------
# Transformer utilities
# --------------------------------------------------------------------------------------------------------------
def add_position(x: np.ndarray, signal: np.ndarray, t0: int = 0) -> np.ndarray:
    return x + signal[None, t0:t0 + x.shape[1], :]


def time_sum(x):
    return _t(x).sum(dim=1)


def time_sum_grads(shape: Sequence[int], dy):
    """Gradient of ``time_sum`` w.r.t. its [B, T, D] input."""
    x = torch.zeros(*shape, dtype=_t(dy).dtype, requires_grad=True)
    return torch.autograd.grad((time_sum(x) * _t(dy)).sum(), [x])[0]


def unfinished_mask(finished: np.ndarray, dtype=np.float32) -> np.ndarray:
    return np.where(np.asarray(finished) != 0, 0.0, 1.0).astype(dtype)


def log_softmax_from_stats(x: np.ndarray, rmax: np.ndarray, rlse: np.ndarray) -> np.ndarray:
    return (x - rmax[:, None]) - rlse[:, None]


def greedy_update(argmax, finished, end_id: int):
    """One greedy step (decoders/autoregressive.py:461-480): -> (symbols, finished', mask, all_finished)."""
    argmax, finished = np.asarray(argmax), np.asarray(finished)
    sym = np.where(finished != 0, 0, argmax)
    fin = (finished != 0) | (sym == end_id)
    return sym.astype(np.int32), fin.astype(np.int32), (~fin).astype(np.int32), bool(fin.all())


def gemm(a: np.ndarray, b: np.ndarray, trans_a: bool, trans_b: bool) -> np.ndarray:
    return (a.T if trans_a else a) @ (b.T if trans_b else b)
