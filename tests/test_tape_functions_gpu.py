"""The tape functions that only the model tests reached -- the fused cells, the merged NematusGRU step and its hoisted
input projection, the attention pieces, the sentence heads, the convolution + max-pool, the two loss functions and
``Tape.param`` / ``Tape.named_param`` -- against float64 autograd with the harness of tests/tape_ref.py: poisoned buffers,
the per-tensor bound 10 x max(e32, 1e-6 max|f64|), the conditioning gate, every module switch off in turn.

The models call these closures in one arrangement: every operand a parameter or an inner ``Var``, every operand needing
a gradient, one reader each.  The graphs here give each differentiable input a second reader, created once before and
once after the function under test (so its backward meets a fresh destination once and a written one once), make each
operand in turn a constant, and pick the smallest shapes at which each forward route, tail and dispatch branch is taken.

The loss functions return a plain tensor and turn their input into its own gradient buffer; they and the parameter
lookups have tests of their own below, with the same bound.

Run on the closures as they were before these tests, three graphs failed: ``lstm_cell`` with z constant and
``nematus_cell`` with the gates' pre-activation constant dropped the other operands' gradients (their slots were taken
and never written: NaN, or the second reader's contribution alone), and ``attn_energies`` raised on a ``v`` without a
gradient buffer (``None.view``).  The closures now take scratch for the gradient nobody wants and go through
``tape.grad(v)``.  On the MI355X every family stays below 0.04 of its bound (e32 / max|f64| at most 3e-7).
"""
import numpy as np
import pytest
import torch

from . import tape_ref as R
from .test_tape_gpu import _rng, away, i32, rnd, weight

FAMILIES = {}


def case(family, name, build, inputs, **kw):
    c = R.Case(family + "/" + name, build, inputs, **kw)
    FAMILIES.setdefault(family, []).append(c)
    return c


def fanned(family, name, fn, inputs, fans, receives=None, values=None):
    """``fn`` (-> dict of outputs) in a graph where the input ``fan`` has a second reader, created after ``fn``
    ("first") and before it ("last"), for every ``fan`` in ``fans``; a ``fan`` of None: ``fn`` alone.  ``receives``: the
    outputs of ``fn`` that receive a gradient (default: all); the second reader always receives one."""
    rng = _rng(family + name)
    for fan in fans:
        for order in ("first", "last") if fan is not None else ("alone",):
            def build(f, v, fan=fan, order=order):
                outs = {}
                if order == "last":
                    outs["other"] = f.scale(getattr(v, fan), 0.5)
                outs.update(fn(f, v))
                if order == "first":
                    outs["other"] = f.scale(getattr(v, fan), 0.5)
                return outs
            upstream = None
            if receives is not None:
                upstream = dict(receives)
                if fan is not None:
                    upstream["other"] = rnd(rng, *inputs[fan][1].shape)
            case(family, "{}-{}-{}".format(name, fan, order), build, inputs, upstream=upstream, values=values)


def differentiable(inputs):
    return [n for n, (kind, _) in inputs.items() if kind in ("leaf", "param")]


def with_kind(inputs, **kinds):
    return {n: (kinds.get(n, kind), arr) for n, (kind, arr) in inputs.items()}


# ---------------------------------------------------------------------------------- k. the fused cells
ROWS = 5


def _lstm_cases(h):
    fam = "k-lstm-H{}".format(h)
    rng = _rng(fam)
    inputs = {"z": ("leaf", rnd(rng, ROWS, 4 * h)), "c": ("leaf", rnd(rng, ROWS, h))}
    dh, dc = rnd(rng, ROWS, h), rnd(rng, ROWS, h)

    def cell(forget_bias):
        def fn(f, v):
            h_new, c_new = f.lstm_cell(v.z, v.c, forget_bias=forget_bias)
            return {"h": h_new, "c_new": c_new}
        return fn
    for fb in (0.0, 1.0):
        fanned(fam, "both-fb{:g}".format(fb), cell(fb), inputs, ("z", "c"), receives={"h": dh, "c_new": dc})
    fanned(fam, "only-h", cell(1.0), inputs, ("z", "c"), receives={"h": dh})
    fanned(fam, "only-c", cell(1.0), inputs, ("z", "c"), receives={"c_new": dc})
    fanned(fam, "neither", cell(1.0), inputs, ("z", "c"), receives={})
    # z needs no gradient, c_prev does: the backward kernel still wants somewhere to put dz
    fanned(fam, "const-z", cell(1.0), with_kind(inputs, z="const"), ("c", None), receives={"h": dh, "c_new": dc})
    fanned(fam, "const-c", cell(1.0), with_kind(inputs, c="const"), ("z", None), receives={"h": dh, "c_new": dc})
    return fam


LSTM = {h: _lstm_cases(h) for h in (8, 6)}


def _nematus_cell_cases(h):
    fam = "k-nematus-H{}".format(h)
    rng = _rng(fam)
    inputs = {"g": ("leaf", rnd(rng, ROWS, 2 * h)), "sc": ("leaf", rnd(rng, ROWS, h)), "ci": ("leaf", rnd(rng, ROWS, h)),
              "hp": ("leaf", rnd(rng, ROWS, h))}
    fn = lambda f, v: {"h": f.nematus_cell(v.g, v.sc, v.ci, v.hp)}
    fanned(fam, "leaves", fn, inputs, differentiable(inputs))
    for const in inputs:                   # (g: the kernel still wants somewhere to put dg)
        some = with_kind(inputs, **{const: "const"})
        fanned(fam, "const-" + const, fn, some, differentiable(some) + [None])
    return fam


NEMATUS = {h: _nematus_cell_cases(h) for h in (8, 6)}


# ---------------------------------------------------------------------------------- l. the merged NematusGRU step
BLOCKS = ("gi", "ci", "gs", "cs")


def _gru_inputs(rng, h, d, biases=True):
    shapes = {"gi": (d, 2 * h), "ci": (d, h), "gs": (h, 2 * h), "cs": (h, h)}
    inputs = {}
    for key in BLOCKS:
        inputs["w_" + key] = ("param", weight(rng, *shapes[key]))
        if biases:
            inputs["b_" + key] = ("param", rnd(rng, shapes[key][1], scale=0.3))
    return inputs


def _gru_params(v):
    return {key: (getattr(v, "w_" + key), getattr(v, "b_" + key, None)) for key in BLOCKS}


MERGED_SHAPES = ((8, 8, "full"), (8, 6, "state"), (12, 6, "unfused"))


def _merged_cases(h, d, route):
    fam = "l-merged-{}".format(route)
    rng = _rng(fam)
    inputs = {"x": ("leaf", rnd(rng, ROWS, d)), "hp": ("leaf", rnd(rng, ROWS, h)), **_gru_inputs(rng, h, d)}
    step = lambda f, v: {"h": f.nematus_cell_merged(v.x, v.hp, _gru_params(v), route=route)}
    fanned(fam, "step", step, inputs, ("x", "hp"))
    if route == "full":
        fanned(fam, "const-x", step, with_kind(inputs, x="const"), ("hp", None))
        bare = {"x": inputs["x"], "hp": inputs["hp"], **_gru_inputs(rng, h, d, biases=False)}
        fanned(fam, "no-biases", step, bare, ("x", "hp"))

    # three chained steps that write the rows of one buffer of all steps
    chain_in = {**inputs, "x1": ("leaf", rnd(rng, ROWS, d)), "x2": ("leaf", rnd(rng, ROWS, d))}

    def chain(f, v):
        p = _gru_params(v)
        hs = f.new((3 * ROWS, h))
        state = v.hp
        for t, x in enumerate((v.x, v.x1, v.x2)):
            state = f.nematus_cell_merged(x, state, p, out=f.rows(hs, t * ROWS, (t + 1) * ROWS), route=route)
        return {"hs": hs, "last": f.tanh(state)}
    fanned(fam, "chain-out-rows", chain, chain_in, ("x1", "hp"))

    # the inputs of all steps projected ahead of the loop; every step reads its rows of the projection
    if route != "state":
        proj_in = {"xs": ("leaf", rnd(rng, 3 * ROWS, d)), "hp": inputs["hp"], **_gru_inputs(rng, h, d)}
        proj_route = "state" if route == "full" else route

        def hoisted(f, v):
            p = _gru_params(v)
            xp = f.nematus_input_projection(v.xs, p)
            state = v.hp
            for t in range(3):
                state = f.nematus_cell_merged(None, state, p, x_proj=f.rows(xp, t * ROWS, (t + 1) * ROWS),
                                              route=proj_route)
            return {"h": state, "xp": xp}
        fanned(fam, "x_proj", hoisted, proj_in, ("xs", "hp"),
               receives={"h": rnd(rng, ROWS, h)})            # (the projection's rows belong to the steps: value only)
    return fam


MERGED = {route: _merged_cases(h, d, route) for h, d, route in MERGED_SHAPES}


# ---------------------------------------------------------------------------------- m. attention
BSZ, ATT = 3, 8
MASKS = {1: [[1.0], [0.0], [1.0]],
         5: [[1, 1, 1, 1, 1], [1, 1, 0, 0, 0], [1, 0, 1, 1, 0]],           # the last one: no prefix
         70: [[1.0] * 70, [1.0] * 33 + [0.0] * 37, [1.0, 0.0] * 35]}


def _energy_inputs(rng, slen, rows=BSZ):
    return {"y": ("leaf", rnd(rng, rows, ATT)), "hf": ("leaf", rnd(rng, BSZ * slen, ATT)),
            "v": ("param", rnd(rng, ATT, scale=1.0 / np.sqrt(ATT)))}


def _energies_cases(slen):
    fam = "m-energies-S{}".format(slen)
    rng = _rng(fam)
    inputs = _energy_inputs(rng, slen)
    fn = lambda f, v: {"e": f.attn_energies(v.y, v.hf, v.v, BSZ, slen)}
    fanned(fam, "v-param", fn, inputs, differentiable(inputs))
    leaf_v = with_kind(inputs, v="leaf")           # no gradient buffer until somebody writes one
    fanned(fam, "v-leaf", fn, leaf_v, differentiable(leaf_v) + [None])
    fanned(fam, "const-hf", fn, with_kind(inputs, hf="const"), ("y", "v"))
    fanned(fam, "const-y", fn, with_kind(inputs, y="const"), ("hf", "v"))
    return fam


ENERGIES = {slen: _energies_cases(slen) for slen in (5, 70)}


def _softmax_cases(slen):
    fam = "m-softmax-S{}".format(slen)
    rng = _rng(fam)
    inputs = {"e": ("leaf", rnd(rng, BSZ, slen)), "mask": ("aux", torch.tensor(MASKS[slen], dtype=torch.float32))}
    fanned(fam, "masked", lambda f, v: {"w": f.attn_softmax(v.e, v.mask, BSZ)}, inputs, ("e",))
    fanned(fam, "no-mask", lambda f, v: {"w": f.attn_softmax(v.e, None, BSZ)}, inputs, ("e",))
    fanned(fam, "w_out", lambda f, v: {"w": f.attn_softmax(v.e, v.mask, BSZ, 1, w_out=f.tensor((BSZ, slen)))}, inputs,
           ("e",))
    return fam


SOFTMAX = {slen: _softmax_cases(slen) for slen in (1, 5, 70)}


def _attention_chain():
    slen = 5
    rng = _rng("m-chain")
    inputs = {**_energy_inputs(rng, slen), "vals": ("leaf", rnd(rng, BSZ * slen, ATT)),
              "mask": ("aux", torch.tensor(MASKS[slen], dtype=torch.float32))}

    def fn(f, v):
        e = f.attn_energies(v.y, v.hf, v.v, BSZ, slen)
        w = f.attn_softmax(e, v.mask, BSZ)
        return {"ctx": f.weighted_sum(w, v.vals, BSZ, slen), "w": w}
    fanned("m-chain", "energies-softmax-sum", fn, inputs, differentiable(inputs))


_attention_chain()


def _forward_only_cases():
    """Two queries per sentence: the backward closures assert one, so the values alone."""
    out = []
    for slen in (5, 70):
        rng = _rng("m-k2-{}".format(slen))
        inputs = {**with_kind(_energy_inputs(rng, slen, rows=2 * BSZ), y="const", hf="const", v="const"),
                  "mask": ("aux", torch.tensor(MASKS[slen], dtype=torch.float32))}

        def build(f, v, slen=slen):
            e = f.attn_energies(v.y, v.hf, v.v, BSZ, slen, 2)
            return {"e": e, "w": f.attn_softmax(e, v.mask, BSZ, 2), "plain": f.attn_softmax(e, None, BSZ, 2)}
        out.append(R.Case("m-k2/S{}".format(slen), build, inputs, upstream={}))
    return out


# ---------------------------------------------------------------------------------- n. sentence heads
STEPS = 5
HEAD_MASK = torch.tensor([[1, 1, 1, 1, 1], [0, 0, 1, 0, 0], [1, 1, 1, 0, 0]], dtype=torch.float32)    # one live position


def _head_cases():
    for heads in (1, 4):
        fam = "n-time_softmax-H{}".format(heads)
        inputs = {"e": ("leaf", rnd(_rng(fam), BSZ * STEPS, heads)), "mask": ("aux", HEAD_MASK)}
        fanned(fam, "masked", lambda f, v: {"w": f.time_softmax(v.e, v.mask, BSZ, STEPS)}, inputs, ("e",))
        fanned(fam, "no-mask", lambda f, v: {"w": f.time_softmax(v.e, None, BSZ, STEPS)}, inputs, ("e",))
    rng = _rng("n-heads")
    inputs = {"w": ("leaf", rnd(rng, BSZ * STEPS, 4)), "vals": ("leaf", rnd(rng, BSZ * STEPS, 6))}
    fn = lambda f, v: {"y": f.heads_weighted_sum(v.w, v.vals, BSZ, STEPS)}
    fanned("n-heads", "leaves", fn, inputs, ("w", "vals"))
    fanned("n-heads", "const-w", fn, with_kind(inputs, w="const"), ("vals", None))
    fanned("n-heads", "const-vals", fn, with_kind(inputs, vals="const"), ("w", None))
    chain_in = {"e": ("leaf", rnd(rng, BSZ * STEPS, 4)), "x": ("leaf", rnd(rng, BSZ * STEPS, 6)), "mask": ("aux", HEAD_MASK)}

    def chain(f, v):
        w = f.time_softmax(v.e, v.mask, BSZ, STEPS)
        return {"temporal": f.heads_weighted_sum(w, v.x, BSZ, STEPS), "w": w}
    fanned("n-heads", "chain", chain, chain_in, ("e", "x"))


_head_cases()


# ---------------------------------------------------------------------------------- o. convolution + relu + max-pool
CONV = dict(bsz=2, slen=7, emb=6, filters=((1, 4), (3, 3), (4, 5)))


def _conv_cases():
    rng = _rng("o-conv inputs")
    bsz, slen, emb = CONV["bsz"], CONV["slen"], CONV["emb"]
    inputs = {"x": ("leaf", rnd(rng, bsz * slen, emb)),
              "mask": ("aux", torch.tensor([[1.0] * 7, [1.0] * 4 + [0.0] * 3])), "lengths": ("aux", i32(7, 4))}
    for width, n in CONV["filters"]:
        inputs["w%d" % width] = ("param", weight(rng, width * emb, n).reshape(width, emb, n))
        inputs["b%d" % width] = ("param", rnd(rng, n, scale=0.3))

    def conv(segment, masked):
        def fn(f, v):
            pooled, pmask, plens = f.conv1d_relu_maxpool(
                v.x, [getattr(v, "w%d" % w) for w, _ in CONV["filters"]], [getattr(v, "b%d" % w) for w, _ in CONV["filters"]],
                bsz, slen, segment, mask=v.mask if masked else None, lengths=v.lengths if masked else None)
            assert (pmask is None) == (plens is None) == (not masked)
            if masked:
                f.exact("pooled mask", pmask)
                f.exact("pooled lengths", plens)
            return {"y": pooled}
        return fn
    for segment in (3, 7):                 # 3: S' = 3 pads one position on either side; 7: one window
        for masked in (True, False):
            name = "s{}-{}".format(segment, "masked" if masked else "bare")
            fanned("o-conv", name, conv(segment, masked), inputs, ("x", None))      # (x fanned: accumulate_dx both ways)
        fanned("o-conv", "s{}-const-x".format(segment), conv(segment, True), with_kind(inputs, x="const"), (None,))


_conv_cases()


def _conv_margins(c):
    """(smallest |pre-activation|, smallest lead of a window's positive maximum over its runner-up) in float64."""
    from . import sent_cnn_ref as C
    import torch.nn.functional as TF
    bsz, slen, emb = CONV["bsz"], CONV["slen"], CONV["emb"]
    x = torch.from_numpy(c.inputs["x"][1]).double().view(bsz, slen, emb)
    kink, lead = np.inf, np.inf
    for width, _ in CONV["filters"]:
        w = torch.from_numpy(c.inputs["w%d" % width][1]).double()
        b = torch.from_numpy(c.inputs["b%d" % width][1]).double()
        pad = (width - 1) // 2
        pre = TF.conv1d(TF.pad(x.transpose(1, 2), (pad, width - 1 - pad)), w.permute(2, 1, 0)) + b[None, :, None]
        assert torch.equal(torch.relu(pre), C.conv_relu(x, w, b))
        kink = min(kink, float(pre.abs().min()))
        for segment in (3, 7):
            sp = (slen + segment - 1) // segment
            pb = (sp * segment - slen) // 2
            win = TF.pad(pre, (pb, sp * segment - slen - pb), value=-np.inf).view(bsz, -1, sp, segment)
            top = win.topk(2, -1).values
            live = top[..., 0] > 0
            lead = min(lead, float((top[..., 0] - top[..., 1])[live].min()))
    return kink, lead


# ---------------------------------------------------------------------------------- p. the loss functions
XENT_SIZES = {"6x37-scalar": (6, 37, 37), "6x40-regs8": (6, 40, 40), "6x40-in-43-scalar": (6, 40, 43),
              "2x40000-regs16": (2, 40000, 40000)}
XENT_OPTIONS = [(smoothing, weighted) for smoothing in (0.0, 0.1) for weighted in (True, False)]
GRAD_SCALE = 0.25


def _xent_inputs(size):
    rows, vocab, _ = XENT_SIZES[size]
    rng = _rng("xent" + size)
    x = rnd(rng, rows, vocab)
    targets = rng.integers(0, vocab, rows).astype(np.int32)
    targets[0], targets[-1] = vocab - 1, 0                 # the last and the first class: always inside [0, V)
    weights = rng.uniform(0.5, 1.5, rows).astype(np.float32)
    weights[rows // 2] = 0.0
    return x, targets, weights


def _xent_reference(size, smoothing, weighted, dtype):
    """(loss rows, grad_scale * d sum(loss) / d logits) of tf.losses.softmax_cross_entropy(label_smoothing) per row,
    times the row's weight, in ``dtype``; the gradient by autograd."""
    x, targets, weights = _xent_inputs(size)
    x = torch.from_numpy(x).to(dtype).requires_grad_(True)
    logp = torch.log_softmax(x, -1)
    nll = -logp.gather(1, torch.from_numpy(targets).long()[:, None])[:, 0]
    loss = (1.0 - smoothing) * nll + smoothing * (-logp.mean(1))
    if weighted:
        loss = loss * torch.from_numpy(weights).to(dtype)
    (grad,) = torch.autograd.grad(loss.sum(), [x])
    return loss.detach(), grad * GRAD_SCALE


def _sqerr_inputs(dim):
    rng = _rng("sqerr%d" % dim)
    return rnd(rng, 5, dim), rnd(rng, 5)


def _sqerr_reference(dim, dtype):
    pred, targets = _sqerr_inputs(dim)
    pred = torch.from_numpy(pred).to(dtype).requires_grad_(True)
    loss = ((pred - torch.from_numpy(targets).to(dtype)[:, None]) ** 2).sum(1)
    (grad,) = torch.autograd.grad(loss.sum(), [pred])
    return loss.detach(), grad * GRAD_SCALE


# ---------------------------------------------------------------------------------- q. parameters of a store
class _Store:
    """What ``Tape.param`` / ``Tape.named_param`` ask of ``ctx.store``: the variables by full name and their slices of one
    flat gradient buffer."""

    def __init__(self, arrays, base, device):
        self.values = {n: torch.from_numpy(a).to(device) for n, a in arrays.items()}
        self.flat = torch.from_numpy(base).to(device)
        self.slices, pos = {}, 0
        for n, a in arrays.items():
            self.slices[n] = self.flat[pos:pos + a.size].view(a.shape)
            pos += a.size

    def __getitem__(self, name):
        return self.values[name]

    def g(self, name):
        return self.slices[name]


class _Part:
    name = "head"

    def var_name(self, name):
        return self.name + "/" + name

    def var(self, ctx, name):
        return ctx.store[self.var_name(name)]


def _param_inputs():
    rng = _rng("params")
    arrays = {"head/kernel": weight(rng, 8, 6), "shared/bias": rnd(rng, 6), "head/unused": rnd(rng, 3)}
    base = away(rng, sum(a.size for a in arrays.values()))
    return arrays, base, rnd(rng, 4, 8), rnd(rng, 4, 6)


def _param_reference(dtype):
    """(y, the flat gradient buffer = base + gradient) of y = x . kernel + bias for the upstream gradient dy."""
    arrays, base, x, dy = _param_inputs()
    t = {n: torch.from_numpy(a).to(dtype).requires_grad_(True) for n, a in arrays.items()}
    y = torch.from_numpy(x).to(dtype) @ t["head/kernel"] + t["shared/bias"]
    grads = torch.autograd.grad((y * torch.from_numpy(dy).to(dtype)).sum(), list(t.values()), allow_unused=True)
    flat = torch.cat([(torch.zeros_like(p) if g is None else g).reshape(-1) for p, g in zip(t.values(), grads)])
    return y.detach(), torch.from_numpy(base).to(dtype) + flat


# ---------------------------------------------------------------------------------- host: conditioning, the mirrors
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_graph_is_well_conditioned(family):
    """float32 on the CPU alone stays ten times inside the project's 1e-4 on every compared tensor of every graph."""
    for c in FAMILIES[family]:
        R.check_condition("host/" + family, c)


def test_forward_only_and_loss_cases_are_well_conditioned():
    for c in _forward_only_cases():
        R.check_condition("host/m-k2", c)
    for size in XENT_SIZES:
        for smoothing, weighted in XENT_OPTIONS:
            w64, w32 = (_xent_reference(size, smoothing, weighted, dt) for dt in (torch.float64, torch.float32))
            R.tensor_bound("host/xent", "loss", w64[0], w32[0])
            R.tensor_bound("host/xent", "grad", w64[1], w32[1])
    for dim in (1, 3):
        w64, w32 = (_sqerr_reference(dim, dt) for dt in (torch.float64, torch.float32))
        R.tensor_bound("host/squared_error", "loss", w64[0], w32[0])
        R.tensor_bound("host/squared_error", "grad", w64[1], w32[1])
    w64, w32 = _param_reference(torch.float64), _param_reference(torch.float32)
    R.tensor_bound("host/params", "y", w64[0], w32[0])
    R.tensor_bound("host/params", "flat gradient", w64[1], w32[1])


def test_convolution_inputs_keep_away_from_the_kink_and_from_ties():
    """The kernel and float64 must agree on which side of zero a pre-activation lies and on which position wins a
    window: no pre-activation within 1e-3 of zero, no positive maximum within 1e-3 of its runner-up."""
    kink, lead = _conv_margins(FAMILIES["o-conv"][0])
    assert kink > 1e-3 and lead > 1e-3, (kink, lead)


def test_merged_step_mirror_is_the_cell_on_the_four_products():
    """``RefNS.nematus_cell_merged`` (from the eight tensors) equals oracle/pointwise_ref.py::nematus_cell on the four
    products, with and without biases and with the input half projected ahead."""
    from oracle import pointwise_ref as P
    f = R.RefNS(torch.float64)
    rng = _rng("mirror")
    for h, d, biases in ((8, 8, True), (12, 6, True), (8, 6, False)):
        t = {n: torch.from_numpy(a).double() for n, (_, a) in _gru_inputs(rng, h, d, biases).items()}
        p = {key: (t["w_" + key], t.get("b_" + key)) for key in BLOCKS}
        x, hp = torch.from_numpy(rnd(rng, ROWS, d)).double(), torch.from_numpy(rnd(rng, ROWS, h)).double()
        prod = {key: (x if key[1] == "i" else hp) @ p[key][0] + (0.0 if p[key][1] is None else p[key][1]) for key in BLOCKS}
        want = P.nematus_cell(prod["gs"] + prod["gi"], prod["cs"], prod["ci"], hp)[0]
        assert float((f.nematus_cell_merged(x, hp, p) - want).abs().max()) <= 1e-14
        xp = f.nematus_input_projection(x, p)
        assert torch.equal(xp, torch.cat([prod["gi"], prod["ci"]], 1))
        out = torch.zeros(ROWS, h, dtype=torch.float64)
        got = f.nematus_cell_merged(None, hp, p, x_proj=xp, out=out)
        assert float((got - want).abs().max()) <= 1e-14 and torch.equal(out, got)


# ---------------------------------------------------------------------------------- GPU: the families
def _run_family(dev, monkeypatch, family, label=None):
    for c in FAMILIES[family]:
        R.run_all_settings(dev, monkeypatch, c, label or family)


@pytest.mark.gpu
@pytest.mark.parametrize("h", sorted(LSTM))
def test_lstm_cell(dev, monkeypatch, h):
    """(k) gradients arriving through h', through c', through both and through neither; forget_bias 0 and 1; z or c_prev
    without a gradient -- with z constant the gradient of c_prev must still be written."""
    _run_family(dev, monkeypatch, LSTM[h])


@pytest.mark.gpu
@pytest.mark.parametrize("h", sorted(NEMATUS))
def test_nematus_cell(dev, monkeypatch, h):
    """(k) the four products as leaves and each in turn a constant -- with the gates' pre-activation constant the other
    three gradients must still be written."""
    _run_family(dev, monkeypatch, NEMATUS[h])


@pytest.mark.gpu
@pytest.mark.parametrize("route", [r for _, _, r in MERGED_SHAPES])
def test_nematus_cell_merged(dev, monkeypatch, route):
    """(l) the three forward routes (each call asserts the one that ran), x constant, no biases, three chained steps
    into the rows of one buffer, and the input half projected for all steps ahead of the loop."""
    _run_family(dev, monkeypatch, MERGED[route])


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["FUSED_FULL_STEP", "FUSED_STATE_STEP"])
def test_nematus_cell_merged_with_a_fusion_switched_off(dev, monkeypatch, switch):
    """(l) the shape that takes the full step, one route further down."""
    from neuralmonkey_amd import autodiff
    monkeypatch.setattr(autodiff, switch, False)
    want = "state" if switch == "FUSED_FULL_STEP" else "unfused"
    for c in FAMILIES[MERGED["full"]]:
        run = R.run_tape(dev, c)
        assert run.routes and set(run.routes) == {want}, (c.name, run.routes)
        R.check("l merged, {} off".format(switch), c, run, R.Refs(c))


@pytest.mark.gpu
@pytest.mark.parametrize("slen", sorted(ENERGIES))
def test_attn_energies(dev, monkeypatch, slen):
    """(m) v a parameter slice and v a leaf without a buffer of its own; keys or query constant."""
    _run_family(dev, monkeypatch, ENERGIES[slen])


@pytest.mark.gpu
@pytest.mark.parametrize("slen", sorted(SOFTMAX))
def test_attn_softmax(dev, monkeypatch, slen):
    """(m) masks that differ per sentence (one of them no prefix), no mask, the weights in a tensor of the caller's."""
    _run_family(dev, monkeypatch, SOFTMAX[slen])


@pytest.mark.gpu
def test_attention_chain(dev, monkeypatch):
    """(m) energies -> softmax -> weighted sum as attention/combination.py and coverage.py build it."""
    _run_family(dev, monkeypatch, "m-chain")


@pytest.mark.gpu
def test_two_queries_per_sentence_forward(dev):
    """(m) rows_per_key = 2: energies, masked and plain softmax -- the values (the backward closures take one query)."""
    for c in _forward_only_cases():
        run = R.run_tape(dev, c, backward=False)
        R.check_values("m rows_per_key 2", run, R.Refs(c))


@pytest.mark.gpu
def test_sentence_heads(dev, monkeypatch):
    """(n) time_softmax with 1 and 4 heads, masked (one row with a single live position) and not; heads_weighted_sum with
    either operand read twice or constant; the two chained as encoders/attentive.py does."""
    for family in ("n-time_softmax-H1", "n-time_softmax-H4", "n-heads"):
        _run_family(dev, monkeypatch, family, "n heads")


@pytest.mark.gpu
def test_conv1d_relu_maxpool(dev, monkeypatch):
    """(o) widths 1, 3, 4 over S = 7 with segments 3 (padded on both sides) and 7; pooled mask and lengths bit for bit;
    x read twice (accumulate_dx on and off) and x constant; filter and bias gradients on non-zero bases."""
    _run_family(dev, monkeypatch, "o-conv")


# ---------------------------------------------------------------------------------- GPU: losses and parameters
def _xent_on_tape(dev, size, smoothing, weighted, recording):
    """-> (loss rows, the [rows, V] logits after the call, the whole buffer, the Var)."""
    from neuralmonkey_amd import autodiff as F
    rows, vocab, ld = XENT_SIZES[size]
    x, targets, weights = _xent_inputs(size)
    wide = torch.full((rows, ld), float("nan"), device=dev)
    wide[:, :vocab] = torch.from_numpy(x).to(dev)
    tape = F.Tape(R.PoisonCtx(dev), "xent", recording=recording)
    var = tape.leaf(wide[:, :vocab], needs_grad=True)
    loss = F.xent(tape, var, torch.from_numpy(targets).to(dev), torch.from_numpy(weights).to(dev) if weighted else None,
                  torch.tensor([GRAD_SCALE], device=dev), smoothing)
    R.sync("xent " + size)
    return loss.cpu(), wide[:, :vocab].cpu(), wide.cpu(), var


@pytest.mark.gpu
@pytest.mark.parametrize("size", sorted(XENT_SIZES))
def test_xent_overwrites_the_logits_with_their_gradient(dev, size):
    """(p) the scalar kernel (V % 4 != 0; a row stride of 43), the 8- and the 16-register kernel, each with label
    smoothing 0 and 0.1 and with and without weights (one of them zero): the loss rows, ``logits.grad is logits.data``,
    the gradient scaled by grad_scale; nothing written past the V columns; a tape that does not record leaves the
    logits as they were."""
    rows, vocab, ld = XENT_SIZES[size]
    x = torch.from_numpy(_xent_inputs(size)[0])
    for smoothing, weighted in XENT_OPTIONS:
        w64, w32 = (_xent_reference(size, smoothing, weighted, dt) for dt in (torch.float64, torch.float32))
        label = "p xent {} s{:g} {}".format(size, smoothing, "weighted" if weighted else "unweighted")
        loss, grad, wide, var = _xent_on_tape(dev, size, smoothing, weighted, True)
        assert var.grad is var.data
        R.close(label, "loss", loss, w64[0], w32[0])
        R.close(label, "grad", grad, w64[1], w32[1])
        assert torch.isnan(wide[:, vocab:]).all() and wide[:, vocab:].shape == (rows, ld - vocab)
        loss, after, _, var = _xent_on_tape(dev, size, smoothing, weighted, False)
        assert var.grad is None and not var.needs_grad and torch.equal(after, x)
        R.close(label, "loss (not recording)", loss, w64[0], w32[0])


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 3])
def test_squared_error_overwrites_the_predictions_with_their_gradient(dev, dim):
    """(p) loss rows and grad_scale * 2 (pred - target) in place; no targets: None and nothing touched; a tape that does
    not record leaves the predictions as they were."""
    from neuralmonkey_amd import autodiff as F
    pred, targets = _sqerr_inputs(dim)
    w64, w32 = _sqerr_reference(dim, torch.float64), _sqerr_reference(dim, torch.float32)
    scale = torch.tensor([GRAD_SCALE], device=dev)
    label = "p squared_error dim {}".format(dim)
    for recording in (True, False):
        tape = F.Tape(R.PoisonCtx(dev), "sqerr", recording=recording)
        var = tape.leaf(torch.from_numpy(pred).to(dev), needs_grad=True)
        assert F.squared_error(tape, var, None, scale) is None
        assert var.grad is None and torch.equal(var.data.cpu(), torch.from_numpy(pred))
        loss = F.squared_error(tape, var, torch.from_numpy(targets).to(dev), scale)
        R.sync(label)
        R.close(label, "loss", loss.cpu(), w64[0], w32[0])
        if recording:
            assert var.grad is var.data
            R.close(label, "grad", var.grad.cpu(), w64[1], w32[1])
        else:
            assert var.grad is None and torch.equal(var.data.cpu(), torch.from_numpy(pred))


@pytest.mark.gpu
def test_param_and_named_param_are_slices_of_the_flat_gradient(dev):
    """(q) a product over ``Tape.param`` (a part's variable) and ``Tape.named_param`` (a full store name): the flat buffer
    ends as its base + the gradients, a variable nobody read keeps its base bit for bit; on a tape that does not record
    the Vars have no gradient."""
    from neuralmonkey_amd import autodiff as F
    arrays, base, x, dy = _param_inputs()
    w64, w32 = _param_reference(torch.float64), _param_reference(torch.float32)
    for recording in (True, False):
        ctx = R.PoisonCtx(dev)
        ctx.store = store = _Store(arrays, base, dev)
        tape = F.Tape(ctx, "params", recording=recording)
        kernel, bias = tape.param(_Part(), "kernel"), tape.named_param("shared/bias")
        assert kernel.data is store["head/kernel"] and bias.data is store["shared/bias"]
        y = F.linear(tape, tape.leaf(torch.from_numpy(x).to(dev)), kernel, bias)
        if not recording:
            assert kernel.grad is None and bias.grad is None and not kernel.needs_grad and not bias.needs_grad
        else:
            assert kernel.grad.data_ptr() == store.g("head/kernel").data_ptr()
            assert bias.grad.data_ptr() == store.g("shared/bias").data_ptr()
            R.seed_grad(y, torch.from_numpy(dy).to(dev))
            tape.backward()
        R.sync("params")
        R.close("q params", "y", y.data.cpu(), w64[0], w32[0])
        flat = store.flat.cpu()
        if recording:
            R.close("q params", "flat gradient", flat, w64[1], w32[1])
        else:
            assert torch.equal(flat, torch.from_numpy(base))
        assert torch.equal(flat[-3:], torch.from_numpy(base)[-3:])
