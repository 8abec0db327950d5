"""Float64 mirrors of the autodiff tape's functions and a harness that evaluates ONE graph description three times: on a
``Tape`` over the HIP kernels, in float64 torch autograd (the reference) and in float32 torch autograd on the CPU (what
float32 arithmetic alone costs on that graph -- the per-tensor tolerance comes from it).

A graph is a function ``build(f, v)``: ``f`` is a namespace of the tape functions (``TapeNS`` or ``RefNS``), ``v`` a
namespace of the graph's inputs; it returns a dict of named outputs.  Functions that write in place on the tape
(``add_``, ``linear(out=, accumulate=True)``, ``rowscale(out=, accumulate=True)``) RETURN the updated handle and the
builder goes on with what they return; ``out=`` without ``accumulate`` writes through a handle from ``f.new`` / ``f.cols``.

Inputs are ``(kind, array)``:
  "param"  Var(data, <buffer that holds a random non-zero base>, True): expected buffer = base + gradient;
  "leaf"   tape.leaf(data, needs_grad=True): ``grad`` stays None until somebody writes it;
  "const"  tape.leaf(data, needs_grad=False): nothing may be allocated or written for it;
  "aux"    a plain tensor (ids, lengths, masks, position signals).

Where a tape function's signature needs plumbing that a graph description should not repeat, ``TapeNS`` has an adapter
and ``RefNS`` a mirror of the same signature: the merged NematusGRU step takes the four kernels and four biases
({"gi", "ci", "gs", "cs"} -> (kernel, bias or None)) and the adapter concatenates them as nn/cells.py does;
``f.tensor`` is a tensor of the caller's (None in the reference); ``f.exact(name, t)`` names a side result that is no
``Var`` and is compared bit for bit.

With NM_TAPE_STATS=<path> in the environment the largest e32 / max|f64| and the largest GPU error / bound seen under each
label (``STATS``) are written to that file as JSON when the process ends: the figures a pull request reports.
"""
import atexit
import json
import os
import types
import zlib
from contextlib import contextmanager

import numpy as np
import torch

SWITCHES = ("ALIAS_ADD_GRADS", "LAZY_ADD", "GROUP_WGRADS", "CHAIN_WGRADS", "ZERO_ARENA", "FUSED_LN_BWD")
SETTINGS = (None,) + SWITCHES          # everything on, then each switch off alone

INT_SENTINEL = 0x3F3F3F3F

# label -> [largest e32 / max|f64|, largest GPU error / bound] over the tensors compared under that label
STATS = {}


def _dump_stats():
    path = os.environ.get("NM_TAPE_STATS")
    if path and STATS:
        with open(path, "w", encoding="utf-8") as fh:
            json.dump(STATS, fh, indent=1, sort_keys=True)


atexit.register(_dump_stats)


# ------------------------------------------------------------------------------------------------ the poisoning context
class _Session:
    """What a tape asks of a session: a ``__dict__`` for the arenas and the device-side step counter."""

    def __init__(self, device):
        self.device = device
        self._step = None

    def step_tensor(self):
        if self._step is None:
            self._step = torch.full((1,), 3, dtype=torch.int32, device=self.device)
        return self._step


class PoisonCtx:
    """A run context whose buffers behave like ``Session.buffer`` -- persistent per (key, shape, dtype), cleared only on
    request -- and are POISONED where the session's merely hold the previous step's values: every request without
    ``zero`` fills a float buffer with NaN and an int buffer with a large sentinel, so a kernel that accumulates into a
    buffer it should overwrite, or reads scratch before writing it, shows up as NaN in a result."""

    def __init__(self, device):
        self.device = device
        self.session = _Session(device)
        self.buffers = {}
        self.requests = []          # (key, shape, dtype, zero) of every request, in order

    def buffer(self, key, shape, dtype=torch.float32, zero=False, zero_init=False):
        shape = tuple(int(s) for s in shape)
        full = (key, shape, dtype)
        self.requests.append((key, shape, dtype, zero))
        buf = self.buffers.get(full)
        created = buf is None
        if created:
            buf = self.buffers[full] = torch.empty(shape, dtype=dtype, device=self.device)
        if zero or (zero_init and created):
            buf.zero_()
        elif not zero_init:
            buf.fill_(float("nan") if dtype.is_floating_point else INT_SENTINEL)
        return buf


# ------------------------------------------------------------------------------------------------ the two namespaces
class TapeNS:
    """The tape functions with the tape bound: handles are ``Var``s."""

    def __init__(self, tape):
        from neuralmonkey_amd import autodiff
        self.F = autodiff
        self.tape = tape
        self.masks = []             # of every dropout call, in order: where the forward output is not zero
        self.exacts = {}            # name -> side result compared bit for bit (``exact``)
        self.routes = []            # the forward route of every nematus_cell_merged call that named one

    def __getattr__(self, name):
        fn = getattr(self.F, name)
        return lambda *a, **k: fn(self.tape, *a, **k)

    def new(self, shape):
        return self.tape.new(shape)

    def cols(self, v, lo, hi):
        return self.tape.cols(v, lo, hi)

    def rows(self, v, lo, hi):
        return self.tape.rows(v, lo, hi)

    def dropout(self, x, keep_prob, salt):
        out = self.F.dropout(self.tape, x, keep_prob, True, salt)
        self.masks.append((out.data != 0).cpu())
        return out

    def sdp_attention(self, q, k, v, mask, heads, b, tq, tk):
        return self.F.sdp_attention(self.tape, q, k, v, mask, heads, b, tq, b, tk)

    def exact(self, name, t):
        """A side result that is no ``Var`` (a pooled mask, pooled lengths): compared with the reference's bit for bit."""
        self.exacts[name] = t.detach().cpu().double()

    def tensor(self, shape):
        """A tensor of the caller's (``w_out=``): poisoned like every other buffer."""
        return torch.full(tuple(shape), float("nan"), device=self.tape.ctx.device)

    def attn_softmax(self, e, mask, bsz, rows_per_key=1, w_out=None):
        w = self.F.attn_softmax(self.tape, e, mask, bsz, rows_per_key, w_out)
        if w_out is not None:
            assert w.data.data_ptr() == w_out.data_ptr(), "attn_softmax did not write the caller's tensor"
        return w

    def _merged(self, p):
        """What nn/cells.py keeps per run context: [W_gi | W_ci], [W_gs | W_cs] and the concatenated biases."""
        def cat(a, b, dim):
            kernels = [p[a][0].data, p[b][0].data]
            biases = None if p[a][1] is None else torch.cat([p[a][1].data.reshape(-1), p[b][1].data.reshape(-1)])
            return torch.cat(kernels, dim).contiguous(), biases
        return cat("gi", "ci", 1) + cat("gs", "cs", 1)

    def nematus_input_projection(self, x_all, p):
        w_in, b_in, _, _ = self._merged(p)
        return self.F.nematus_input_projection(self.tape, x_all, w_in, b_in, p)

    def nematus_cell_merged(self, x, h_prev, p, x_proj=None, out=None, route=None):
        """``route``: the forward route the case's shapes select ("full", "state" or "unfused").  Asserted twice: from
        ``ops.nematus_state_step_ok`` / ``nematus_full_step_ok`` on the very tensors, and from the launch that ran (with
        a module switch off: the next route down)."""
        from neuralmonkey_amd import ops
        w_in, b_in, w_st, b_st = self._merged(p)
        names = ("nematus_full_step", "nematus_state_step", "nematus_cell_fwd")
        saved = {n: getattr(ops, n) for n in names}
        ran = []
        for n in names:
            setattr(ops, n, lambda *a, _n=n, **k: (ran.append(_n), saved[_n](*a, **k))[1])
        try:
            h_new = self.F.nematus_cell_merged(self.tape, x, h_prev, w_in, b_in, w_st, b_st, p, x_proj=x_proj, out=out)
        finally:
            for n in names:
                setattr(ops, n, saved[n])
        if route is not None:
            state_ok = ops.nematus_state_step_ok(h_prev.data, w_st, h_new.data)
            full_ok = state_ok and x_proj is None and ops.nematus_full_step_ok(x.data, w_in)
            assert ("full" if full_ok else "state" if state_ok else "unfused") == route, (route, state_ok, full_ok)
            if route == "full" and not self.F.FUSED_FULL_STEP:
                route = "state"
            if route != "unfused" and not self.F.FUSED_STATE_STEP:
                route = "unfused"
            want = {"full": "nematus_full_step", "state": "nematus_state_step", "unfused": "nematus_cell_fwd"}[route]
            assert ran == [want], (ran, want)
            self.routes.append(route)
        return h_new


class RefNS:
    """The same functions over torch tensors of one dtype, differentiable by autograd."""

    def __init__(self, dtype, masks=None):
        self.dtype = dtype
        self.masks = masks
        self.exacts = {}
        self._n_drop = 0

    def _aux(self, t):
        return t.to(self.dtype) if t.dtype.is_floating_point else t.long()

    @staticmethod
    def _put(out, y, accumulate):
        if out is None:
            return y
        if accumulate:
            return out + y
        out.copy_(y)
        return out

    def new(self, shape):
        return torch.zeros(tuple(shape), dtype=self.dtype)

    def cols(self, v, lo, hi):
        return v[:, lo:hi]

    def rows(self, v, lo, hi):
        return v[lo:hi]

    def linear(self, x, w, b=None, out=None, accumulate=False, trans_b=False, act=None):
        y = x @ (w.t() if trans_b else w)
        if b is not None:
            y = y + b
        if act is not None:
            y = {"relu": torch.relu, "tanh": torch.tanh}[act](y)
        return self._put(out, y, accumulate)

    def linear_multi(self, x, ws):
        return [x @ w for w in ws]

    def sigmoid(self, x, shift=0.0):
        return torch.sigmoid(x + shift)

    def tanh(self, x):
        return torch.tanh(x)

    def relu(self, x):
        return torch.relu(x)

    def scale(self, x, alpha):
        return x * alpha

    def copy(self, x, out=None):
        return self._put(out, x * 1.0, False)

    def add_scalar(self, x, alpha):
        return x + alpha

    def add(self, a, b):
        return a + b

    def add_(self, acc, x):
        return acc + x

    def mul(self, a, b):
        return a * b

    def div(self, a, b):
        return a / b

    def blend(self, u, h, c):
        return u * h + (1 - u) * c

    def dropout(self, x, keep_prob, salt):          # pylint: disable=unused-argument
        if self.masks is None:       # no tape at hand (the host's conditioning check): any fixed mask will do
            gen = torch.Generator().manual_seed(1000 + self._n_drop)
            mask = torch.rand(x.shape, generator=gen) < keep_prob
        else:
            mask = self.masks[self._n_drop]
        self._n_drop += 1
        return x * mask.to(self.dtype) / keep_prob

    def concat(self, parts):
        return torch.cat(list(parts), 1)

    def embedding(self, table, ids, out=None, mask_pad=False, scale_by=1.0):
        ids = self._aux(ids).reshape(-1)
        y = table[ids] * scale_by
        if mask_pad:
            y = y * (ids != 0).to(self.dtype)[:, None]
        return self._put(out, y, False)

    def layer_norm(self, x, gamma, beta, eps=1e-6):
        mean = x.mean(-1, keepdim=True)
        var = ((x - mean) ** 2).mean(-1, keepdim=True)
        return (x - mean) * torch.rsqrt(var + eps) * gamma + beta

    def add_layer_norm(self, a, x, gamma, beta, eps=1e-6):
        total = a + x
        return total, self.layer_norm(total, gamma, beta, eps)

    def rnn_select(self, h_new, h_prev, lengths, t, y_out):
        live = (t < self._aux(lengths)).to(self.dtype)[:, None]
        if y_out is not None:
            y_out.copy_(live * h_new)
        return live * h_new + (1 - live) * h_prev

    def reverse_sequence(self, x, lengths):
        b, s, _ = x.shape
        lens = self._aux(lengths).clamp(max=s)[:, None]
        pos = torch.arange(s)[None, :].expand(b, s)
        src = torch.where(pos < lens, lens - 1 - pos, pos)
        return torch.gather(x, 1, src[:, :, None].expand_as(x))

    def maxout(self, x, pool=2):
        groups = x.shape[1] // pool
        best = x[:, :groups]
        for k in range(1, pool):            # the first maximal member takes the gradient
            nxt = x[:, k * groups:(k + 1) * groups]
            best = torch.where(nxt > best, nxt, best)
        return best

    def sdp_attention(self, q, k, v, mask, heads, b, tq, tk):
        from tests.test_transformer_gpu import _sdp_ref
        d = q.shape[1]
        ctx, _ = _sdp_ref(q.view(b, tq, d), k.view(b, tk, d), v.view(b, tk, d), self._aux(mask), heads, d // heads,
                          False, 1.0, 1, 0)
        return ctx.reshape(b * tq, d)

    def rowscale(self, x, s, out=None, accumulate=False):
        return self._put(out, x * s, accumulate)

    def weighted_sum(self, w, vals, bsz, slen, rows_per_key=1):
        k = rows_per_key
        w3 = w.view(bsz, k, w.shape[1])[:, :, :slen]
        return (w3 @ vals.view(bsz, slen, -1)).reshape(bsz * k, -1)

    def add_position(self, x, signal, bsz, steps, t0=0):
        d = x.shape[1]
        return (x.view(bsz, steps, d) + self._aux(signal)[t0:t0 + steps]).reshape(bsz * steps, d)

    def add_position_param(self, x, table, bsz, steps):
        d = x.shape[1]
        return (x.view(bsz, steps, d) + table[:steps]).reshape(bsz * steps, d)

    def add_row(self, x, row):
        return x + row.reshape(1, -1)

    def time_sum(self, x, bsz, steps):
        return x.view(bsz, steps, -1).sum(1)

    def exact(self, name, t):
        self.exacts[name] = t.detach().double()

    def tensor(self, shape):             # pylint: disable=unused-argument
        return None

    def lstm_cell(self, z, c_prev, forget_bias=1.0):
        from oracle import pointwise_ref as P
        c_new, h_new, _ = P.lstm_cell(z, c_prev, forget_bias)
        return h_new, c_new

    def nematus_cell(self, g_pre, sc, ci, h_prev):
        from oracle import pointwise_ref as P
        return P.nematus_cell(g_pre, sc, ci, h_prev)[0]

    @staticmethod
    def _product(x, wb):
        w, b = wb
        return x @ w if b is None else x @ w + b.reshape(1, -1)

    def nematus_input_projection(self, x_all, p):
        return torch.cat([self._product(x_all, p["gi"]), self._product(x_all, p["ci"])], 1)

    def nematus_cell_merged(self, x, h_prev, p, x_proj=None, out=None, route=None):      # pylint: disable=unused-argument
        """The step from the four kernels and four biases themselves (nn/ortho_gru_cell.py:73-105), so that autograd
        yields THEIR gradients.  With ``out=`` the result is copied into the caller's rows and the chain goes on with
        the result itself (a later write into other rows of that buffer must not invalidate what autograd saved)."""
        h = h_prev.shape[1]
        xp = x_proj if x_proj is not None else self.nematus_input_projection(x, p)
        gates = torch.sigmoid(xp[:, :2 * h] + self._product(h_prev, p["gs"]))
        r, u = gates[:, :h], gates[:, h:]
        cand = torch.tanh(xp[:, 2 * h:] + r * self._product(h_prev, p["cs"]))
        y = u * h_prev + (1 - u) * cand
        if out is not None:
            out.copy_(y)
        return y

    def attn_energies(self, y, hf, v, bsz, slen, rows_per_key=1):
        a = y.shape[1]
        pre = y.view(bsz, rows_per_key, 1, a) + hf.view(bsz, 1, slen, a)
        return (torch.tanh(pre) * v.reshape(-1)).sum(-1).reshape(bsz * rows_per_key, slen)

    def attn_softmax(self, e, mask, bsz, rows_per_key=1, w_out=None):                   # pylint: disable=unused-argument
        from oracle import pointwise_ref as P
        if mask is None:
            return torch.softmax(e, -1)
        return P.attn_softmax(e, P.mask_rows(self._aux(mask), e.shape[0], bsz, rows_per_key))

    def time_softmax(self, e, mask, bsz, steps):
        """tests/pool_ref.py::time_softmax in torch: softmax over T, times the mask, divided by (sum + 1e-8)."""
        h = e.shape[1]
        w = torch.softmax(e.view(bsz, steps, h), 1)
        if mask is not None:
            u = w * self._aux(mask)[:, :, None]
            w = u / (u.sum(1, keepdim=True) + 1e-8)
        return w.reshape(bsz * steps, h)

    def heads_weighted_sum(self, w, vals, bsz, steps):
        h, d = w.shape[1], vals.shape[1]
        return (w.view(bsz, steps, h).transpose(1, 2) @ vals.view(bsz, steps, d)).reshape(bsz * h, d)

    def conv1d_relu_maxpool(self, x, filters, biases, bsz, slen, segment, mask=None, lengths=None):
        from . import sent_cnn_ref as C
        x3 = x.view(bsz, slen, -1)
        pooled = torch.cat([C.same_max_pool(C.conv_relu(x3, w, b), segment) for w, b in zip(filters, biases)], 1)
        pmask = None if mask is None else C.same_max_pool(self._aux(mask)[:, None, :], segment)[:, 0]
        plens = None if lengths is None else (self._aux(lengths) + segment - 1) // segment
        return pooled.transpose(1, 2).reshape(-1, pooled.shape[1]), pmask, plens


# ------------------------------------------------------------------------------------------------ one graph, three times
class Case:
    """A graph description.  ``upstream``: name -> array for the outputs that receive a gradient; by default every
    output gets a random one.  ``values``: the outputs whose VALUE is compared (reading a value computes a pending sum, so a
    sum that nobody may read is left out); by default all.  ``adjacent``: tuples of "param" names whose tensors lie back
    to back in one flat buffer."""

    def __init__(self, name, build, inputs, upstream=None, values=None, adjacent=()):
        self.name, self.build, self.inputs = name, build, inputs
        self.upstream, self.values, self.adjacent = upstream, values, adjacent
        self.seed = zlib.crc32(name.encode())

    def base(self, name):
        rng = np.random.default_rng([self.seed, zlib.crc32(name.encode())])
        return torch.from_numpy(rng.uniform(0.5, 1.5, self.inputs[name][1].shape).astype(np.float32)
                                * rng.choice([-1.0, 1.0], self.inputs[name][1].shape).astype(np.float32))

    def upstream_for(self, name, shape):
        if self.upstream is not None:
            g = self.upstream.get(name)
            return None if g is None else torch.as_tensor(g, dtype=torch.float32)
        rng = np.random.default_rng([self.seed, 7, zlib.crc32(name.encode())])
        return torch.from_numpy(rng.standard_normal(tuple(shape)).astype(np.float32))


def seed_grad(v, g):
    """Hand the caller's gradient ``g`` to the output ``v`` the way the models do (``logits.grad = ...``)."""
    if v.grad is None:
        v.grad = g
    elif v.fresh:
        v.grad.copy_(g)
        v.fresh = False
    else:
        v.grad.add_(g)


def run_tape(dev, case, ctx=None, key="tape_ref", recording=True, backward=True):
    """Build ``case`` on a tape under a ``PoisonCtx`` and run its backward pass.  -> TapeRun with ``values`` / ``grads``
    (host tensors; the gradient of a "param" is its whole buffer, base included; of a "leaf" None if nobody wrote it)."""
    from neuralmonkey_amd import autodiff as F
    run = types.SimpleNamespace()
    run.ctx = ctx if ctx is not None else PoisonCtx(dev)
    run.tape = tape = F.Tape(run.ctx, key, recording=recording)
    flat = {}
    for group in case.adjacent:
        total = sum(case.inputs[n][1].size for n in group)
        buf = torch.empty(total, device=dev)
        pos = 0
        for n in group:
            arr = case.inputs[n][1]
            flat[n] = buf[pos:pos + arr.size].view(arr.shape)
            pos += arr.size
    run.vars = {}
    for name, (kind, arr) in case.inputs.items():
        if kind == "aux":
            t = torch.as_tensor(arr)
            run.vars[name] = t.to(dev)
            continue
        data = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).to(dev)
        if name in flat:
            flat[name].copy_(data)
            data = flat[name]
        if kind == "param":
            run.vars[name] = F.Var(data, case.base(name).to(dev) if recording else None, recording)
        else:
            run.vars[name] = tape.leaf(data, needs_grad=(kind == "leaf"))
    ns = TapeNS(tape)
    run.outs = outs = case.build(ns, types.SimpleNamespace(**run.vars))
    run.masks, run.exacts, run.routes = ns.masks, ns.exacts, ns.routes
    names = case.values if case.values is not None else list(outs)
    run.values = {n: outs[n].data.detach().cpu().clone() for n in names}
    run.grads = {}
    if recording and backward:
        run.upstream = {}
        for n, o in outs.items():
            g = case.upstream_for(n, o.shape)
            if g is not None:
                run.upstream[n] = g.to(dev)
                seed_grad(o, run.upstream[n])
        tape.backward()
        assert not tape._wgrads and not tape._chains and not tape._ops        # pylint: disable=protected-access
        for name, (kind, _) in case.inputs.items():
            if kind == "aux":
                continue
            g = run.vars[name].grad
            if kind == "const":
                assert g is None, "a gradient buffer for {}, which needs none".format(name)
            run.grads[name] = None if g is None else g.detach().cpu().clone()
    sync(case.name)
    return run


def sync(what):
    """Wait for the device; a device error ends the pytest run: nothing more may run on this GPU in this session."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        import pytest
        pytest.exit("device error in {}: {}".format(what, err), returncode=3)


def run_ref(case, dtype, masks=None, exacts=None):
    """-> (values, grads, pure): ``grads`` of a "param" is base + gradient computed in ``dtype``; ``pure`` the gradient
    alone (where it is exactly zero nobody touched the buffer).  ``exacts``: a dict that receives the side results the
    graph named with ``f.exact``.  A case in which no output receives a gradient has zero gradients."""
    leaves, handles = {}, {}
    for name, (kind, arr) in case.inputs.items():
        if kind == "aux":
            handles[name] = torch.as_tensor(arr)
            continue
        t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).to(dtype)
        if kind != "const":
            t.requires_grad_(True)
            leaves[name] = t
        handles[name] = t
    ns = RefNS(dtype, masks)
    outs = case.build(ns, types.SimpleNamespace(**handles))
    if exacts is not None:
        exacts.update(ns.exacts)
    names = case.values if case.values is not None else list(outs)
    values = {n: outs[n].detach().clone() for n in names}
    loss = None
    for n, o in outs.items():
        g = case.upstream_for(n, o.shape)
        if g is not None:
            term = (o * g.to(dtype)).sum()
            loss = term if loss is None else loss + term
    got = [None] * len(leaves) if loss is None else torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    grads, pure = {}, {}
    for (name, t), g in zip(leaves.items(), got):
        g = torch.zeros_like(t) if g is None else g
        pure[name] = g
        grads[name] = case.base(name).to(dtype) + g if case.inputs[name][0] == "param" else g
    return values, grads, pure


class Refs:
    def __init__(self, case, masks=None):
        self.masks = masks
        self.exacts = {}
        self.v64, self.g64, self.pure = run_ref(case, torch.float64, masks, self.exacts)
        self.v32, self.g32, _ = run_ref(case, torch.float32, masks)


def tensor_bound(label, name, w64, w32):
    """The tolerance of one compared tensor: 10 x max(e32, 1e-6 max|f64|) with e32 what float32 on the CPU loses on the same
    graph.  The graph must be conditioned well enough for that to stay inside the project's float32 tolerance."""
    scale = float(w64.abs().max()) if w64.numel() else 0.0
    e32 = float((w32.double() - w64).abs().max()) if w64.numel() else 0.0
    bound = 10.0 * max(e32, 1e-6 * scale)
    assert bound <= 1e-4 * max(scale, 1.0), \
        "{} / {}: ill-conditioned graph: float32 on the CPU is off by {:.3g} at scale {:.3g}".format(label, name, e32, scale)
    stat = STATS.setdefault(label, [0.0, 0.0])
    stat[0] = max(stat[0], e32 / scale if scale else 0.0)
    return bound


def check_condition(label, case, refs=None):
    """The host's part of the tolerance: every compared tensor of ``case`` meets the conditioning bound."""
    refs = refs if refs is not None else Refs(case)
    for n, w in refs.v64.items():
        tensor_bound(label, "value " + n, w, refs.v32[n])
    for n, w in refs.g64.items():
        tensor_bound(label, "grad " + n, w, refs.g32[n])
    return refs


def close(label, name, got, w64, w32):
    bound = tensor_bound(label, name, w64, w32)
    assert tuple(got.shape) == tuple(w64.shape), (label, name, got.shape, w64.shape)
    assert not torch.isnan(got).any(), "{} / {}: NaN".format(label, name)
    err = float((got.double() - w64).abs().max()) if w64.numel() else 0.0
    stat = STATS[label]
    stat[1] = max(stat[1], err / bound if bound else 0.0)
    assert err <= bound, "{} / {}: off by {:.3g}, bound {:.3g} (e32 {:.3g})".format(
        label, name, err, bound, float((w32.double() - w64).abs().max()))


def check_values(label, run, refs):
    """The values of the tape run against float64 under the per-tensor bound, the side results bit for bit."""
    for n, got in run.values.items():
        close(label, "value " + n, got, refs.v64[n], refs.v32[n])
    assert set(run.exacts) == set(refs.exacts), (label, sorted(run.exacts), sorted(refs.exacts))
    for n, got in run.exacts.items():
        assert torch.equal(got, refs.exacts[n]), "{} / {}: {} instead of {}".format(label, n, got, refs.exacts[n])


def check(label, case, run, refs):
    """Every value and gradient of the tape run against float64 under the per-tensor bound; what float64 leaves exactly
    zero (rows nobody touched) must be exactly the base, or exactly zero, on the tape."""
    check_values(label, run, refs)
    for n, w64 in refs.g64.items():
        got = run.grads[n]
        kind = case.inputs[n][0]
        if got is None:
            assert kind == "leaf" and not refs.pure[n].any(), "{} / grad {}: never written".format(label, n)
            continue
        close(label, "grad " + n, got, w64, refs.g32[n])
        untouched = refs.pure[n] == 0
        rest = case.base(n) if kind == "param" else torch.zeros_like(got)
        assert torch.equal(got[untouched], rest[untouched]), "{} / grad {}: an untouched element moved".format(label, n)


@contextmanager
def setting(monkeypatch, name):
    """Everything on (None) or the module switch ``name`` off."""
    from neuralmonkey_amd import autodiff
    with monkeypatch.context() as m:
        if name is not None:
            m.setattr(autodiff, name, False)
        yield


def run_graph(dev, build, inputs, upstream=None, values=None, adjacent=(), name="graph"):
    """Evaluate one graph on the tape (under ``PoisonCtx``) and in float64 / float32 autograd.
    -> ((values, grads) of the tape, (values, grads) in float64, (values, grads) in float32)."""
    case = Case(name, build, inputs, upstream, values, adjacent)
    run = run_tape(dev, case)
    refs = Refs(case, run.masks)
    return (run.values, run.grads), (refs.v64, refs.g64), (refs.v32, refs.g32)


def run_all_settings(dev, monkeypatch, case, label=None):
    """``case`` with everything on and with each switch off in turn; every setting must meet the bound."""
    label = label or case.name
    refs = None
    for name in SETTINGS:
        with setting(monkeypatch, name):
            run = run_tape(dev, case)
        if refs is None:
            refs = Refs(case, run.masks)
        else:
            assert all(torch.equal(a, b) for a, b in zip(run.masks, refs.masks))
        try:
            check(label, case, run, refs)
        except AssertionError as err:
            raise AssertionError("[{}, {} off] {}".format(case.name, name, err)) from err
    return refs
