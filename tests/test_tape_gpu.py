"""The autodiff tape's own mechanics against float64 autograd: which buffer a gradient kernel writes, and whether it
overwrites or accumulates (``grad_slot`` / ``fresh``, the aliased and lazy ``add``, the layer norm's backward routes,
deferred / grouped / chained weight and bias gradients, ``linear_multi``, the zeroing of ``sdp_attention``, the zero
arena, inference tapes), with the plain tape functions needed to drive them.

Every graph is described once (tests/tape_ref.py) and evaluated on a ``Tape`` under a context whose buffers are
persistent and POISONED (NaN / a sentinel unless ``zero=True``), in float64 autograd and in float32 autograd on the CPU.
Tolerance per compared tensor: 10 x max(e32, 1e-6 max|f64|), e32 = max|float32 on the CPU - float64| on the same graph;
the helper asserts that this bound stays within 1e-4 x max(max|f64|, 1) (``test_every_graph_is_well_conditioned`` does
so on the host for every graph), so no graph passes by widening its own bound.  Each graph runs with every module
switch on and with each one off in turn.

``TAPE_TESTS`` says for every tape function which test runs it on a ``Tape``: a test here or a test elsewhere (the fused
cells, the attention pieces, the sentence heads, the convolution, the losses and the parameter lookups:
tests/test_tape_functions_gpu.py).  No function is left to the model tests alone.
"""
import inspect
import itertools
import zlib

import numpy as np
import pytest
import torch

from . import tape_ref as R

FAMILIES = {}


def case(family, name, build, inputs, **kw):
    c = R.Case(family + "/" + name, build, inputs, **kw)
    FAMILIES.setdefault(family, []).append(c)
    return c


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def rnd(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def away(rng, *shape):
    """O(1) values that keep away from zero."""
    return (rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def weight(rng, k, n):
    return rnd(rng, k, n, scale=1.0 / np.sqrt(k))


def i32(*vals):
    return torch.tensor(vals, dtype=torch.int32)


# ---------------------------------------------------------------------------------- a. overwrite versus accumulate
B, T, D = 2, 3, 8
CONSUMERS = {
    "linear": lambda f, v, x: f.linear(x, v.w, v.b),
    "tanh": lambda f, v, x: f.tanh(x),
    "layer_norm": lambda f, v, x: f.layer_norm(x, v.gamma, v.beta),
    "dropout": lambda f, v, x: f.dropout(x, 0.7, 1234),
    "add_position_param": lambda f, v, x: f.add_position_param(x, v.table, B, T),
}


def _fanout(order, variant):
    def build(f, v):
        x = v.x0 if variant == "leaf" else f.scale(v.x0, 0.5)
        outs = {}
        if variant == "view":            # the view allocates (and zeroes) x's gradient: every consumer accumulates
            outs["view"] = f.cols(x, 2, 6)
        for n in order:
            outs[n] = CONSUMERS[n](f, v, x)
        return outs
    rng = _rng("fanout")
    inputs = {"x0": ("leaf", away(rng, B * T, D)), "w": ("param", weight(rng, D, D)), "b": ("param", rnd(rng, D)),
              "gamma": ("param", away(rng, D)), "beta": ("param", rnd(rng, D)), "table": ("param", rnd(rng, 5, D))}
    return case("a", "{}-{}".format(variant, ">".join(order)), build, inputs)


FANOUT = {}
for _variant in ("inner", "leaf", "view"):
    for _n in (1, 2, 3):
        FANOUT[_variant, _n] = [_fanout(order, _variant) for subset in itertools.combinations(CONSUMERS, _n)
                                for order in itertools.permutations(subset)]


def _self_pairs():
    rng = _rng("self")
    for variant in ("leaf", "inner"):
        pick = (lambda f, v: v.a) if variant == "leaf" else (lambda f, v: f.scale(v.a, 0.5))
        inputs = {"a": ("leaf", (rng.uniform(0.5, 1.5, (5, 6))).astype(np.float32)),
                  "c": ("const", rng.uniform(1.0, 2.0, (5, 6)).astype(np.float32))}

        def mul(f, v, pick=pick):
            a = pick(f, v)
            return {"y": f.mul(a, a)}

        def add(f, v, pick=pick):
            a = pick(f, v)
            return {"y": f.add(a, a), "z": f.tanh(a)}

        def div(f, v, pick=pick):
            a = pick(f, v)
            return {"y": f.div(a, f.add(a, v.c))}
        for name, build in (("mul(a,a)", mul), ("add(a,a)", add), ("div(a,a+c)", div)):
            case("a-self", variant + "-" + name, build, inputs)


_self_pairs()


# ---------------------------------------------------------------------------------- b. add
def _chain(name, rows, d, first, mixer, strided=False):
    rng = _rng("chain" + name)
    inputs = {"x0": ("leaf", rnd(rng, rows, d))}
    for i in range(4):
        inputs["g%d" % i] = ("param", away(rng, d))
        inputs["b%d" % i] = ("param", rnd(rng, d))
        if mixer == "linear" and i < 3:
            inputs["w%d" % i] = ("param", weight(rng, d, d + 8 if strided else d))

    def build(f, v):
        x = v.x0
        outs = {}
        for i in range(3):
            if i > 0 and first == "tanh":            # somebody else reads the sum before the layer norm: Var.data
                outs["t%d" % i] = f.tanh(x)
            n = f.layer_norm(x, getattr(v, "g%d" % i), getattr(v, "b%d" % i))
            y = f.linear(n, getattr(v, "w%d" % i)) if mixer == "linear" else f.tanh(n)
            if strided:                              # a column view: an operand the one-pass sum + norm does not take
                y = f.cols(y, 0, d)
            x = f.add(x, y)
        outs["top"] = f.layer_norm(x, v.g3, v.b3)
        outs["sum"] = x
        return outs
    return case("b", name, build, inputs)


_chain("chain-ln-first", 16, 16, "ln", "linear")
_chain("chain-tanh-first", 16, 16, "tanh", "linear")
_chain("chain-7x14", 7, 14, "ln", "linear")
_chain("chain-5x2052", 5, 2052, "ln", "tanh")
_chain("chain-strided", 16, 16, "ln", "linear", strided=True)


def _unread_sum(f, v):
    return {"s": f.add(f.tanh(v.x), f.scale(v.x, 0.5))}


case("b", "sum-read-by-nobody", _unread_sum, {"x": ("leaf", rnd(_rng("unread"), 6, 8))}, values=[])


def _add_then_add_(f, v):
    a = f.scale(v.x, 1.5)
    s = f.add(a, v.y)
    a = f.add_(a, v.z)                    # the sum is that of the operands as they were when it was taken
    return {"s": s, "a": a}


case("b", "add-then-add_", _add_then_add_, {k: ("leaf", rnd(_rng("add_" + k), 6, 8)) for k in "xyz"})


def _add_then_accumulating_linear(f, v):
    o = f.linear(v.x, v.w)
    s = f.add(o, v.y)
    o = f.linear(v.z, v.w2, out=o, accumulate=True)
    return {"s": s, "o": f.tanh(o)}


def _add_then_accumulating_rowscale(f, v):
    o = f.rowscale(v.x, v.r)
    s = f.add(o, v.y)
    o = f.rowscale(v.z, v.r2, out=o, accumulate=True)
    return {"s": s, "o": f.tanh(o)}


def _settle_inputs():
    rng = _rng("settle")
    return {"x": ("leaf", rnd(rng, 6, 8)), "y": ("leaf", rnd(rng, 6, 8)), "z": ("leaf", rnd(rng, 6, 8)),
            "w": ("param", weight(rng, 8, 8)), "w2": ("param", weight(rng, 8, 8)), "r": ("leaf", rnd(rng, 6, 1)),
            "r2": ("leaf", rnd(rng, 6, 1))}


case("b", "add-then-accumulating-linear", _add_then_accumulating_linear, _settle_inputs())
case("b", "add-then-accumulating-rowscale", _add_then_accumulating_rowscale, _settle_inputs())


# ---------------------------------------------------------------------------------- c. layer norm backward routes
def _ln(rows, d, mode):
    rng = _rng("ln{}x{}".format(rows, d))
    pk = "const" if mode.startswith("const_gamma") else "param"
    inputs = {"x": ("const" if mode == "const_x" else "leaf", rnd(rng, rows, d)),
              "gamma": (pk, away(rng, d)), "beta": (pk, rnd(rng, d))}

    def build(f, v):
        n = f.layer_norm(v.x, v.gamma, v.beta)
        if mode.endswith("residual"):      # the sum's backward runs first and leaves its gradient in x's buffer
            return {"y": f.add(v.x, f.tanh(n))}
        return {"y": n}
    return case("c", "{}x{}-{}".format(rows, d, mode), build, inputs)


for _rows, _d in ((33, 512), (7, 14), (5, 2052)):
    for _mode in ("fresh", "residual", "const_x", "const_gamma", "const_gamma_residual"):
        _ln(_rows, _d, _mode)


# ---------------------------------------------------------------------------------- d. deferred weight / bias gradients
def _products(name, specs, shapes, views=()):
    """``specs``: (x, w, bias or None, trans_b) per product; ``shapes``: name -> (kind, shape)."""
    rng = _rng("wg" + name)
    inputs = {}
    for n, (kind, shape) in shapes.items():
        inputs[n] = (kind, weight(rng, *shape) if (len(shape) == 2 and shape[0] < 1024) else rnd(rng, *shape))

    def build(f, v):
        outs = {}
        for i, (x, w, b, trans_b) in enumerate(specs):
            xv = f.cols(getattr(v, x), 0, 32) if x in views else getattr(v, x)
            outs["y%d" % i] = f.linear(xv, getattr(v, w), None if b is None else getattr(v, b), trans_b=trans_b)
        return outs
    return case("d-group", name, build, inputs)


_X = lambda *names: {n: ("leaf", (1024, 32)) for n in names}
_products("lone", [("x1", "w1", "b1", False)], {**_X("x1"), "w1": ("param", (32, 48)), "b1": ("param", (48,))})
_products("three-of-one-shape", [("x1", "w1", "b1", False), ("x2", "w2", None, False), ("x1", "w3", None, False)],
          {**_X("x1", "x2"), "w1": ("param", (32, 48)), "w2": ("param", (32, 48)), "w3": ("param", (32, 48)),
           "b1": ("param", (48,))})
_products("two-shapes", [("x1", "w1", None, False), ("x1", "u1", None, False), ("x2", "w2", None, False),
                         ("x2", "u2", None, False)],
          {**_X("x1", "x2"), "w1": ("param", (32, 48)), "w2": ("param", (32, 48)), "u1": ("param", (32, 64)),
           "u2": ("param", (32, 64))})
_products("tied-three-times", [("x1", "w", "b", False), ("x2", "w", "b", False), ("x3", "w", "b", False),
                               ("x1", "w2", None, False)],
          {**_X("x1", "x2", "x3"), "w": ("param", (32, 48)), "w2": ("param", (32, 48)), "b": ("param", (48,))})
_products("trans_b", [("x1", "w1", None, True), ("x2", "w2", "b", True)],
          {**_X("x1", "x2"), "w1": ("param", (48, 32)), "w2": ("param", (48, 32)), "b": ("param", (48,))})
_products("refused-n46", [("x1", "w1", "b1", False), ("x1", "w2", None, False)],
          {**_X("x1"), "w1": ("param", (32, 46)), "w2": ("param", (32, 46)), "b1": ("param", (46,))})
_products("refused-row-stride", [("wide", "w1", None, False), ("wide", "w2", None, False)],
          {"wide": ("leaf", (1024, 35)), "w1": ("param", (32, 48)), "w2": ("param", (32, 48))}, views=("wide",))


def _loop(steps, rows_list):
    rng = _rng("loop")
    inputs = {"w": ("param", weight(rng, 8, 8)), "b": ("param", rnd(rng, 8)), "w6": ("param", weight(rng, 8, 6)),
              "b6": ("param", rnd(rng, 6))}
    for r in rows_list:
        inputs["h%d" % r] = ("leaf", rnd(rng, r, 8))

    def build(f, v):
        outs = {}
        for r in rows_list:
            h = getattr(v, "h%d" % r)
            for _ in range(steps):          # one kernel and one bias for every step and both batches
                h = f.tanh(f.linear(h, v.w, v.b))
                outs["n%d_%d" % (r, _)] = f.linear(h, v.w6, v.b6)        # a bias of width 6: the immediate column sum
            outs["h%d" % r] = h
        return outs
    return case("d-chain", "T{}-rows{}".format(steps, "+".join(map(str, rows_list))), build, inputs)


for _steps in (1, 2, 9):
    _loop(_steps, (16, 48))
_loop(3, (7,))
_loop(2, (16, 7, 48))


# ---------------------------------------------------------------------------------- e. linear
def _linear_cases():
    rng = _rng("linear")
    inputs = {"x": ("leaf", rnd(rng, 6, 8)), "x2": ("leaf", rnd(rng, 6, 5)), "w1": ("param", weight(rng, 8, 4)),
              "w2": ("param", weight(rng, 8, 8)), "b2": ("param", rnd(rng, 8)), "w3": ("param", weight(rng, 5, 8)),
              "w4": ("param", weight(rng, 8, 8))}

    def out_view(f, v):
        wide = f.new((6, 12))
        f.linear(v.x, v.w1, out=f.cols(wide, 0, 4))
        f.linear(v.x, v.w2, v.b2, out=f.cols(wide, 4, 12))
        return {"y": f.tanh(wide)}

    def accumulate(f, v):
        o = f.linear(v.x, v.w2, v.b2)
        o = f.linear(v.x2, v.w3, out=o, accumulate=True)
        return {"y": f.tanh(o)}

    def relu(f, v):
        y = f.linear(v.x, v.w2, v.b2, act="relu")
        return {"y": y, "z": f.linear(y, v.w4), "t": f.tanh(y)}
    case("e", "out-into-a-column-view", out_view, inputs)
    case("e", "accumulate", accumulate, inputs)
    case("e", "relu-epilogue", relu, inputs)


_linear_cases()


# ---------------------------------------------------------------------------------- f. linear_multi
def _multi(name, adjacent, source):
    rng = _rng("multi")
    inputs = {"x0": ("leaf", rnd(rng, 10, 8)), "wq": ("param", weight(rng, 8, 8)), "wk": ("param", weight(rng, 8, 8)),
              "wv": ("param", weight(rng, 8, 8))}

    def build(f, v):
        x = v.x0 if source == "leaf" else f.scale(v.x0, 0.5)
        q, k, _ = f.linear_multi(x, [v.wq, v.wk, v.wv])        # the third projection: consumed by nobody
        return {"q": f.tanh(q), "k": f.cols(k, 2, 6), "x": f.tanh(x)}
    return case("f", name, build, inputs, adjacent=(("wq", "wk", "wv"),) if adjacent else ())


for _adj in (True, False):
    for _src in ("leaf", "inner"):
        _multi("{}-{}".format("batched" if _adj else "fallback", _src), _adj, _src)


# ---------------------------------------------------------------------------------- g. sdp_attention zeroing
def _sdp(name):
    b, t, heads, d = 2, 5, 2, 8
    rng = _rng("sdp")
    inputs = {"x": ("leaf", rnd(rng, b * t, d)), "mask": ("aux", torch.tensor([[1.0] * 5, [1, 1, 1, 0, 0]]))}
    for n in ("wq", "wk", "wv"):
        inputs[n] = ("param", weight(rng, d, d))

    def build(f, v):
        q, k = f.linear(v.x, v.wq), f.linear(v.x, v.wk)
        val = k if name == "k-is-v" else f.linear(v.x, v.wv)
        att = f.sdp_attention(q, k, val, v.mask, heads, b, t, t)
        if name == "k-feeds-a-residual":       # the sum's backward runs first: k accumulates, q and v are fresh
            return {"y": f.add(att, k)}
        return {"y": att}
    return case("g", name, build, inputs)


for _name in ("flags-agree", "k-feeds-a-residual", "k-is-v"):
    _sdp(_name)


# ---------------------------------------------------------------------------------- h. the plain functions
def _plain(name, fn, inputs, fan="x"):
    """``fn`` in a graph where its input ``fan`` has a second reader, created before and after it (so that ``fn``'s
    backward meets a fresh destination once and a written one once)."""
    for order in ("first", "last"):
        def build(f, v, order=order):
            outs = {}
            if order == "last":
                outs["other"] = f.scale(getattr(v, fan), 0.5)
            got = fn(f, v)
            outs.update(got if isinstance(got, dict) else {"y": got})
            if order == "first":
                outs["other"] = f.scale(getattr(v, fan), 0.5)
            return outs
        case("h", "{}-{}".format(name, order), build, inputs)


def _plain_cases():
    rng = _rng("plain")
    x = {"x": ("leaf", away(rng, 6, 8))}
    _plain("sigmoid-shift", lambda f, v: f.sigmoid(v.x, 1.0), x)
    _plain("tanh", lambda f, v: f.tanh(v.x), x)
    _plain("relu", lambda f, v: f.relu(v.x), x)
    _plain("scale", lambda f, v: f.scale(v.x, -1.75), x)
    _plain("add_scalar", lambda f, v: f.tanh(f.add_scalar(v.x, 0.25)), x)

    def copy_out(f, v):
        wide = f.new((6, 16))
        f.copy(v.x, out=f.cols(wide, 0, 8))
        f.copy(f.tanh(v.x), out=f.cols(wide, 8, 16))
        return f.tanh(wide)
    _plain("copy-out", copy_out, x)
    xy = {"x": ("leaf", away(rng, 6, 8)), "y": ("leaf", away(rng, 6, 8)), "u": ("leaf", rng.uniform(0.1, 0.9, (6, 8))
                                                                               .astype(np.float32))}
    _plain("mul", lambda f, v: f.mul(v.x, v.y), xy)
    _plain("div", lambda f, v: f.div(v.x, v.y), xy)
    _plain("div-denominator", lambda f, v: f.div(v.x, v.y), xy, fan="y")
    _plain("blend", lambda f, v: f.blend(v.u, v.x, v.y), xy)
    _plain("blend-gate", lambda f, v: f.blend(v.u, v.x, v.y), xy, fan="u")
    parts = {"x": ("leaf", rnd(rng, 6, 3)), "p": ("leaf", rnd(rng, 6, 8)), "q": ("const", rnd(rng, 6, 5)),
             "r": ("leaf", rnd(rng, 6, 5))}
    _plain("concat-3-8-5", lambda f, v: f.tanh(f.concat([v.x, v.p, v.r])), parts)
    _plain("concat-const-part", lambda f, v: f.tanh(f.concat([v.x, v.p, v.q])), parts)
    emb = {"table": ("param", rnd(rng, 9, 8)), "ids": ("aux", i32(3, 0, 3, 7, 1, 3, 0, 8)), "x": ("leaf", rnd(rng, 8, 8))}
    _plain("embedding", lambda f, v: f.mul(f.embedding(v.table, v.ids), v.x), emb)
    _plain("embedding-mask-pad-scale", lambda f, v: f.mul(f.embedding(v.table, v.ids, mask_pad=True, scale_by=2.5), v.x),
           emb)
    sel = {"x": ("leaf", rnd(rng, 4, 8)), "p": ("leaf", rnd(rng, 4, 8)), "pc": ("const", rnd(rng, 4, 8)),
           "lengths": ("aux", i32(0, 3, 5, 2))}

    def select_y(f, v):
        y = f.new((4, 8))
        return {"h": f.rnn_select(v.x, v.p, v.lengths, 2, y), "y": y}

    def select_y_only(f, v):               # only the emitted row receives a gradient: nothing for the carried state
        y = f.new((4, 8))
        f.rnn_select(v.x, v.pc, v.lengths, 2, y)
        return {"y": y}
    _plain("rnn_select", lambda f, v: f.rnn_select(v.x, v.p, v.lengths, 2, None), sel)
    _plain("rnn_select-prev", lambda f, v: f.rnn_select(v.x, v.p, v.lengths, 2, None), sel, fan="p")
    _plain("rnn_select-y_out", select_y, sel)
    _plain("rnn_select-y_out-only", select_y_only, sel)
    _plain("rnn_select-last-step", lambda f, v: f.rnn_select(v.x, v.p, v.lengths, 4, None), sel)
    rev = {"x": ("leaf", rnd(rng, 3, 4, 8)), "lengths": ("aux", i32(0, 4, 2))}
    _plain("reverse_sequence", lambda f, v: f.reverse_sequence(v.x, v.lengths), rev)
    mx = rnd(rng, 5, 8)
    mx[:, 5] = mx[:, 1]                     # a tie: the first member takes the gradient
    mx[2, 6] = mx[2, 2]
    _plain("maxout-tie", lambda f, v: f.maxout(v.x, 2), {"x": ("leaf", mx)})
    rs = {"x": ("leaf", rnd(rng, 6, 8)), "y": ("leaf", rnd(rng, 6, 8)), "s": ("leaf", rnd(rng, 6, 1)),
          "s2": ("leaf", rnd(rng, 6, 1))}

    def rowscale_acc(f, v):
        o = f.new((6, 8))
        f.rowscale(v.x, v.s, out=o)
        return f.tanh(f.rowscale(v.y, v.s2, out=o, accumulate=True))
    _plain("rowscale", lambda f, v: f.rowscale(v.x, v.s), rs)
    _plain("rowscale-weights", lambda f, v: f.rowscale(v.x, v.s), rs, fan="s")
    _plain("rowscale-out-accumulate", rowscale_acc, rs)
    bsz, slen, a = 3, 5, 8
    ws = {"x": ("leaf", rnd(rng, bsz, slen)), "wide": ("leaf", rnd(rng, bsz, 7)), "w2": ("leaf", rnd(rng, bsz * 2, slen)),
          "vals": ("leaf", rnd(rng, bsz * slen, a)), "steps": ("leaf", rnd(rng, 70 * bsz, slen))}

    def outer_chain(f, v):                  # 70 steps over one leaf: two launches of the chained outer product
        acc = f.weighted_sum(f.rows(v.steps, 0, bsz), v.vals, bsz, slen)
        for t in range(1, 70):
            acc = f.add_(acc, f.weighted_sum(f.rows(v.steps, t * bsz, (t + 1) * bsz), v.vals, bsz, slen))
        return {"y": acc, "z": f.weighted_sum(v.x, v.vals, bsz, slen)}
    _plain("weighted_sum-outer-chain", outer_chain, ws)
    _plain("weighted_sum-values", lambda f, v: f.weighted_sum(v.x, v.vals, bsz, slen), ws, fan="vals")
    _plain("weighted_sum-rows_per_key", lambda f, v: f.weighted_sum(v.w2, v.vals, bsz, slen, 2), ws, fan="w2")
    _plain("weighted_sum-inner-values", lambda f, v: f.weighted_sum(v.x, f.tanh(v.vals), bsz, slen), ws)
    _plain("weighted_sum-short-slen", lambda f, v: f.weighted_sum(v.wide, v.vals, bsz, slen), ws, fan="wide")
    pos = {"x": ("leaf", rnd(rng, B * T, D)), "signal": ("aux", torch.from_numpy(rnd(rng, 10, D))),
           "row": ("param", rnd(rng, 1, D))}
    _plain("add_position-t0", lambda f, v: f.tanh(f.add_position(v.x, v.signal, B, T, t0=4)), pos)
    _plain("add_row", lambda f, v: f.tanh(f.add_row(v.x, v.row)), pos)
    _plain("time_sum", lambda f, v: f.tanh(f.time_sum(v.x, B, T)), pos)
    _plain("dropout", lambda f, v: f.dropout(v.x, 0.6, 77), x)


_plain_cases()


def _cases(*families):
    return [c for fam in families for c in FAMILIES[fam]]


ALL_CASES = [c for cases in FAMILIES.values() for c in cases]


# ---------------------------------------------------------------------------------- host: conditioning, registry
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_graph_is_well_conditioned(family):
    """float32 on the CPU alone stays ten times inside the project's 1e-4 on every compared tensor of every graph."""
    for c in FAMILIES[family]:
        R.check_condition("host/" + family, c)


def test_arena_and_inference_graphs_are_well_conditioned():
    for c in _arena_graphs() + [_caller_owned_case(), _tanh_epilogue_case(), R.Case("e/partly-written", *_partly_written())]:
        R.check_condition("host/custom", c)
    _inference_reference()


# every public function of autodiff that takes a tape, and every public method of Tape: the test of THIS module that
# runs it, or the node id of a test elsewhere that runs it on a Tape
TAPE_TESTS = {
    "Tape.rewind": "test_inference_tape_reuses_two_slots",
    "Tape.buf": "test_zero_arena_rolls_over_and_forgets_the_previous_step",
    "Tape.new": "test_linear_paths",
    "Tape.leaf": "test_fanout_overwrites_once_then_accumulates",
    "Tape.param": "tests/test_tape_functions_gpu.py::test_param_and_named_param_are_slices_of_the_flat_gradient",
    "Tape.named_param": "tests/test_tape_functions_gpu.py::test_param_and_named_param_are_slices_of_the_flat_gradient",
    "Tape.grad": "test_fanout_overwrites_once_then_accumulates",
    "Tape.grad_slot": "test_fanout_overwrites_once_then_accumulates",
    "Tape.view": "test_fanout_overwrites_once_then_accumulates",
    "Tape.cols": "test_fanout_overwrites_once_then_accumulates",
    "Tape.rows": "test_plain_functions",
    "Tape.record": "test_inference_tape_reuses_two_slots",
    "Tape.backward": "test_fanout_overwrites_once_then_accumulates",
    "Tape.settle": "test_add_paths",
    "Tape.defer_wgrad": "test_grouped_weight_gradients",
    "Tape.defer_bias": "test_chained_weight_and_bias_gradients",
    "Tape.flush_wgrads": "test_chained_weight_and_bias_gradients",
    "linear": "test_linear_paths",
    "linear_multi": "test_linear_multi",
    "sigmoid": "test_plain_functions",
    "tanh": "test_plain_functions",
    "relu": "test_plain_functions",
    "scale": "test_plain_functions",
    "copy": "test_plain_functions",
    "add": "test_add_paths",
    "add_": "test_add_paths",
    "mul": "test_plain_functions",
    "div": "test_plain_functions",
    "add_scalar": "test_plain_functions",
    "blend": "test_plain_functions",
    "dropout": "test_plain_functions",
    "concat": "test_plain_functions",
    "embedding": "test_plain_functions",
    "layer_norm": "test_layer_norm_backward_routes",
    "add_layer_norm": "test_inference_tape_reuses_two_slots",
    "rnn_select": "test_plain_functions",
    "reverse_sequence": "test_plain_functions",
    "maxout": "test_plain_functions",
    "sdp_attention": "test_sdp_attention_zeroes_what_is_fresh",
    "rowscale": "test_plain_functions",
    "weighted_sum": "test_plain_functions",
    "add_position": "test_plain_functions",
    "add_position_param": "test_fanout_overwrites_once_then_accumulates",
    "add_row": "test_plain_functions",
    "time_sum": "test_plain_functions",
    "highway": "tests/test_sentence_cnn_gpu.py::test_highway_layer_matches_float64",
    "conv1d_glu": "tests/test_convs2s_kernels_gpu.py::test_taped_encoder_functions_match_float64_autograd",
    "time_max": "tests/test_convs2s_kernels_gpu.py::test_taped_encoder_functions_match_float64_autograd",
    "ctc_loss": "tests/test_ctc_kernels_gpu.py::test_autodiff_op_overwrites_the_logits_with_their_gradient",
    "label_xent": "tests/test_label_kernels_gpu.py::test_autodiff_op_overwrites_the_logits_with_their_gradient",
    "lstm_cell": "tests/test_tape_functions_gpu.py::test_lstm_cell",
    "nematus_cell": "tests/test_tape_functions_gpu.py::test_nematus_cell",
    "nematus_input_projection": "tests/test_tape_functions_gpu.py::test_nematus_cell_merged",
    "nematus_cell_merged": "tests/test_tape_functions_gpu.py::test_nematus_cell_merged",
    "attn_energies": "tests/test_tape_functions_gpu.py::test_attn_energies",
    "attn_softmax": "tests/test_tape_functions_gpu.py::test_attn_softmax",
    "xent": "tests/test_tape_functions_gpu.py::test_xent_overwrites_the_logits_with_their_gradient",
    "squared_error": "tests/test_tape_functions_gpu.py::test_squared_error_overwrites_the_predictions_with_their_gradient",
    "conv1d_relu_maxpool": "tests/test_tape_functions_gpu.py::test_conv1d_relu_maxpool",
    "time_softmax": "tests/test_tape_functions_gpu.py::test_sentence_heads",
    "heads_weighted_sum": "tests/test_tape_functions_gpu.py::test_sentence_heads",
}


def test_every_tape_function_is_in_the_registry():
    import importlib
    import os
    from neuralmonkey_amd import autodiff
    names = set()
    for name, fn in vars(autodiff).items():
        if inspect.isfunction(fn) and not name.startswith("_") and fn.__module__ == autodiff.__name__:
            params = list(inspect.signature(fn).parameters)
            if params and params[0] == "tape":
                names.add(name)
    for name, fn in vars(autodiff.Tape).items():
        if inspect.isfunction(fn) and not name.startswith("_"):
            names.add("Tape." + name)
    assert names == set(TAPE_TESTS), (sorted(names - set(TAPE_TESTS)), sorted(set(TAPE_TESTS) - names))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name, where in TAPE_TESTS.items():
        assert not where.startswith("model tests only"), (name, where)
        if "::" in where:
            path, test = where.split("::")
            assert os.path.isfile(os.path.join(root, path)), (name, where)
            module = importlib.import_module(path[:-3].replace("/", "."))
            assert callable(getattr(module, test)), (name, where)
        else:
            assert callable(globals().get(where)), (name, where)


# ---------------------------------------------------------------------------------- GPU: the families
def _run_cases(dev, monkeypatch, cases, label):
    for c in cases:
        R.run_all_settings(dev, monkeypatch, c, label)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,n", sorted(FANOUT))
def test_fanout_overwrites_once_then_accumulates(dev, monkeypatch, variant, n):
    """(a) a Var read by n consumers in every replay order: the first contribution overwrites a poisoned buffer, the
    others add to it; with a column view taken first every consumer adds to the zeroed buffer."""
    _run_cases(dev, monkeypatch, FANOUT[variant, n], "a fanout {} x{}".format(variant, n))


@pytest.mark.gpu
def test_one_var_as_both_operands(dev, monkeypatch):
    """(a) mul(a, a), add(a, a), div(a, a + c)."""
    _run_cases(dev, monkeypatch, _cases("a-self"), "a self")


@pytest.mark.gpu
def test_add_paths(dev, monkeypatch):
    """(b) residual chains (lazy sum consumed by the layer norm, or forced by another reader; shapes the one-pass kernel
    refuses), a sum read by nobody, add followed by add_ on its operand."""
    _run_cases(dev, monkeypatch, _cases("b"), "b add")


def _caller_owned_case():
    def build(f, v):
        a = f.tanh(v.x)
        extra = f.scale(a, 2.0)                # replayed after the sum's closure: added to whatever a's buffer is by then
        return {"s": f.add(a, f.scale(v.y, 0.5)), "extra": extra, "a": a}       # (a: handed back, no gradient of its own)
    rng = _rng("owned")
    return R.Case("b/caller-owned-gradient", build, {"x": ("leaf", rnd(rng, 6, 8)), "y": ("leaf", rnd(rng, 6, 8))},
                  upstream={"s": rnd(rng, 6, 8), "extra": rnd(rng, 6, 8)}, values=["s", "extra"])


@pytest.mark.gpu
@pytest.mark.parametrize("alias", [True, False])
def test_add_takes_over_a_caller_owned_gradient(dev, monkeypatch, alias):
    """(b) ``add`` documents that the sum's gradient buffer is dead once its closure has run and that the first operand
    without a buffer TAKES IT OVER, later contributions being added to it in place: a tensor the caller set as
    ``out.grad`` ends up as that operand's gradient buffer and holds the operand's FULL gradient.  With ALIAS_ADD_GRADS
    off the caller's tensor is left as it was."""
    from neuralmonkey_amd import autodiff
    c = _caller_owned_case()
    monkeypatch.setattr(autodiff, "ALIAS_ADD_GRADS", alias)
    run = R.run_tape(dev, c)
    a, mine = run.outs["a"], run.upstream["s"]
    g_s, g_extra = (c.upstream_for(n, mine.shape).to(dev) for n in ("s", "extra"))
    full = g_s + 2.0 * g_extra
    if alias:
        assert a.grad.data_ptr() == mine.data_ptr()
        assert float((mine - full).abs().max()) <= 1e-6 * float(full.abs().max())
    else:
        assert a.grad.data_ptr() != mine.data_ptr()
        assert torch.equal(mine, g_s)
        assert float((a.grad - full).abs().max()) <= 1e-6 * float(full.abs().max())
    R.check("b caller-owned", c, run, R.Refs(c))


@pytest.mark.gpu
def test_layer_norm_backward_routes(dev, monkeypatch):
    """(c) fused with a fresh dx, fused onto a residual's gradient, D % 4 != 0, D > 2048, constant gamma / beta, x without
    gradient; gamma / beta gradients on a non-zero base."""
    _run_cases(dev, monkeypatch, _cases("c"), "c layer_norm")


@pytest.mark.gpu
def test_grouped_weight_gradients(dev, monkeypatch):
    """(d) 1024-row products: alone, three of a shape, two shapes, a weight tied over three calls, trans_b, shapes the
    grouped kernel refuses."""
    _run_cases(dev, monkeypatch, _cases("d-group"), "d grouped")


@pytest.mark.gpu
def test_chained_weight_and_bias_gradients(dev, monkeypatch):
    """(d) time loops of 1, 2 and 9 steps over 16 and 48 rows that share one kernel and one bias; 7 rows and a bias of
    width 6 take the immediate paths."""
    _run_cases(dev, monkeypatch, _cases("d-chain"), "d chained")


@pytest.mark.gpu
def test_linear_paths(dev, monkeypatch):
    """(e) out= into column views that fill a wide buffer, accumulate=True, relu in the epilogue with its backward taken
    from the output."""
    _run_cases(dev, monkeypatch, _cases("e"), "e linear")


def _partly_written():
    rng = _rng("partly")

    def build(f, v):
        wide = f.new((6, 12))
        left = f.linear(v.x, v.w, v.b, out=f.cols(wide, 0, 4))
        return {"y": f.tanh(left), "wide": wide}
    inputs = {"x": ("leaf", rnd(rng, 6, 8)), "w": ("param", weight(rng, 8, 4)), "b": ("param", rnd(rng, 4))}
    return build, inputs, {"y": rnd(rng, 6, 4), "wide": None}


@pytest.mark.gpu
def test_columns_nobody_wrote_keep_their_poison(dev):
    """(e) a product written into the first columns of a wide buffer: those columns hold it, the rest is still NaN (nothing
    wrote past the view), and the gradients meet the bound."""
    build, inputs, upstream = _partly_written()
    (values, grads), (v64, g64), (v32, g32) = R.run_graph(dev, build, inputs, upstream, name="e/partly-written")
    assert torch.isnan(values["wide"][:, 4:]).all()
    R.close("e partly written", "value wide[:, :4]", values["wide"][:, :4], v64["wide"][:, :4], v32["wide"][:, :4])
    R.close("e partly written", "value y", values["y"], v64["y"], v32["y"])
    for n in ("x", "w", "b"):
        R.close("e partly written", "grad " + n, grads[n], g64[n], g32[n])


def _tanh_epilogue_case():
    rng = _rng("tanh-epilogue")
    return R.Case("e/tanh-epilogue", lambda f, v: {"y": f.linear(v.x, v.w, v.b, act="tanh")},
                  {"x": ("const", rnd(rng, 6, 8)), "w": ("param", weight(rng, 8, 8)), "b": ("param", rnd(rng, 8))})


@pytest.mark.gpu
def test_tanh_epilogue_is_for_inference_tapes(dev):
    c = _tanh_epilogue_case()
    with pytest.raises(AssertionError, match="only relu has a backward closure"):
        R.run_tape(dev, c)
    run = R.run_tape(dev, c, recording=False)
    refs = R.Refs(c)
    R.close("e tanh epilogue", "value y", run.values["y"], refs.v64["y"], refs.v32["y"])   # pylint: disable=protected-access


@pytest.mark.gpu
def test_linear_multi(dev, monkeypatch):
    """(f) three adjacent kernels (one batched launch) and the same three apart (separate products); a projection nobody
    consumed leaves its weight gradient exactly at its base; one consumed through a view; x read elsewhere too."""
    _run_cases(dev, monkeypatch, _cases("f"), "f linear_multi")


@pytest.mark.gpu
def test_sdp_attention_zeroes_what_is_fresh(dev, monkeypatch):
    """(g) the three accumulate flags agree / k was written by a residual first / k is v."""
    _run_cases(dev, monkeypatch, _cases("g"), "g sdp_attention")


@pytest.mark.gpu
def test_plain_functions(dev, monkeypatch):
    """(h) each plain function with a second reader of its input, replayed before and after it."""
    _run_cases(dev, monkeypatch, _cases("h"), "h plain")


# ---------------------------------------------------------------------------------- i. the zero arena
def _arena_graphs():
    def make(name, rows, d, big_rows):
        rng = _rng("arena" + name)

        def build(f, v):
            y = f.tanh(v.x)
            z = f.mul(y, f.scale(y, 0.5))              # mul adds to zeroed buffers: the arena's
            t = f.tanh(v.big)
            return {"z": f.mul(z, v.x), "big": f.mul(t, t)}
        return R.Case("i/" + name, build, {"x": ("leaf", rnd(rng, rows, d)), "big": ("leaf", rnd(rng, big_rows, d))})
    return [make("A", 33, 96, 50), make("B", 17, 40, 110)]


@pytest.mark.gpu
def test_zero_arena_rolls_over_and_forgets_the_previous_step(dev, monkeypatch):
    """(i) chunks of 4096 floats: graph A (3168-float gradients: one per chunk; a 4800-float one that no chunk holds and
    ``ctx.buffer(zero=True)`` serves), then graph B of other shapes under the same tape key, then A again -- every step
    meets the bound on top of the previous step's gradients, and the chunks stay where they were."""
    from neuralmonkey_amd import autodiff
    monkeypatch.setattr(autodiff._ZeroArena, "CHUNK", 4096)          # pylint: disable=protected-access
    monkeypatch.setattr(autodiff, "ZERO_ARENA", True)
    a, b = _arena_graphs()
    ctx = R.PoisonCtx(dev)
    refs = {c.name: R.Refs(c) for c in (a, b)}
    first = None
    for step, c in enumerate((a, b, a)):
        run = R.run_tape(dev, c, ctx=ctx, key="arena")
        R.check("i arena", c, run, refs[c.name])
        arena = ctx.session._tape_arenas["arena"]                    # pylint: disable=protected-access
        ptrs = [chunk.data_ptr() for chunk in arena.chunks]
        if step == 0:
            first = ptrs
            assert len(ptrs) >= 3, "the graph was to roll over several chunks"
            assert any(zero and shape == (50, 96) for _, shape, _, zero in ctx.requests), "the oversized request"
        assert ptrs[:len(first)] == first
    assert any(zero and shape == (110, 40) for _, shape, _, zero in ctx.requests)


# ---------------------------------------------------------------------------------- j. inference tapes
_INF = dict(rows=4, d=8, steps=4)


def _inference_inputs():
    rng = _rng("inference")
    d = _INF["d"]
    return {"xs": rnd(rng, _INF["steps"], _INF["rows"], d), "h0": rnd(rng, _INF["rows"], d), "wx": weight(rng, d, d),
            "wh": weight(rng, d, d), "b": rnd(rng, d), "gamma": away(rng, d), "beta": rnd(rng, d)}


def _inference_step(f, p, x, h):
    total, normed = f.add_layer_norm(f.linear(x, p["wx"], p["b"]), f.linear(h, p["wh"]), p["gamma"], p["beta"])
    return f.tanh(f.add(normed, f.scale(total, 0.1)))


def _inference_reference():
    out = {}
    arrs = _inference_inputs()
    for dtype in (torch.float64, torch.float32):
        p = {k: torch.from_numpy(v).to(dtype) for k, v in arrs.items()}
        f, h, hs = R.RefNS(dtype), p["h0"], []
        for t in range(_INF["steps"]):
            h = _inference_step(f, p, p["xs"][t], h)
            hs.append(h)
        out[dtype] = hs
    for h64, h32 in zip(out[torch.float64], out[torch.float32]):
        R.tensor_bound("j inference", "h", h64, h32)
    return out


@pytest.mark.gpu
def test_inference_tape_reuses_two_slots(dev, monkeypatch):
    """(j) recording=False: nothing is recorded, no gradient or zeroed buffer is requested, no arena; rewind(0) / rewind(1)
    alternate over four steps and the state of step t-1 is intact after step t; add_layer_norm is one launch."""
    from neuralmonkey_amd import autodiff, ops
    launches = []
    fused = ops.add_layer_norm_fwd
    monkeypatch.setattr(ops, "add_layer_norm_fwd", lambda *a, **k: (launches.append(1), fused(*a, **k))[1])
    want = _inference_reference()
    ctx = R.PoisonCtx(dev)
    tape = autodiff.Tape(ctx, "inference", recording=False)
    f = R.TapeNS(tape)
    p = {k: tape.leaf(torch.from_numpy(v).to(dev)) for k, v in _inference_inputs().items() if k != "xs"}
    xs = torch.from_numpy(_inference_inputs()["xs"]).to(dev)
    h, before = p["h0"], None
    for t in range(_INF["steps"]):
        tape.rewind(t % 2)
        prev = h
        h = _inference_step(f, p, tape.leaf(xs[t]), prev)
        if before is not None:
            assert torch.equal(prev.data, before), "step {} overwrote the state of step {}".format(t, t - 1)
        before = h.data.clone()
        assert h.grad is None and not h.needs_grad
        R.close("j inference", "h{}".format(t), h.data.cpu(), want[torch.float64][t], want[torch.float32][t])  # pylint: disable=protected-access
    assert tape._ops == [] and tape._arena is None and not tape._wgrads and not tape._chains      # pylint: disable=protected-access
    assert len(launches) == _INF["steps"]
    assert not any(zero for *_, zero in ctx.requests)
    slots = {key[2] for key, *_ in ctx.requests}
    assert slots == {0, 1}
    assert len(ctx.buffers) * 2 == len(ctx.requests), "every step of a slot asks for the same buffers again"
