"""The case table of the vocabulary-row kernels of csrc/nm_logits.hip -- nm_row_stats, nm_xent, nm_xent_colsum and
nm_gumbel_argmax -- with their float64 references: tests/test_row_cases_ref.py shows on the CPU that the table reaches
every branch of the three dispatch rules restated below and where the tolerances come from;
tests/test_row_kernels_gpu.py holds the kernels to it.

Layouts.  A case's logits are a [rows, V] view of a flat float32 buffer filled with 3e38: ``plain`` (ldx = V, the view
starts at the aligned base), ``ld1`` (ldx = V + 1), ``shift`` (ldx = V, the view starts one float into the buffer) and
``ld4`` (ldx = V + 4).  For V % 4 == 0 the first is the vector kernel, ``ld1`` and ``shift`` are the scalar kernel by
rule, ``ld4`` stays on the vector kernel with strided rows.  A read of the padding, of the float before a shifted view
or of the four floats behind the last row shows up in the maximum, the argmax and the sums.

Rows are 1 to 7: the kernels take one row per workgroup (the column kernel walks rows g, g + G, ...), so nothing but
the row count itself changes with more of them.

The constants.  E_* are the worst errors of the FLOAT32 NUMPY RESTATEMENT of each operation (f32_stats, f32_xent,
f32_colsum below) against the float64 reference over this table, measured on the CPU by test_row_cases_ref.py -- not
on the kernels.  The kernels sum the same float32 terms in another order and differ from the restatement beyond that
only by the last bits of the device's expf / logf; C_* = about 10 x E_* (the margin tests/sampling_cases.py takes) are
the bounds of the GPU tests.  None is looser than what tests/test_kernels_gpu.py allows (1e-6 for the log-sum-exp, 1e-5
for loss and gradient), with one class apart: see C_LOSS_OFFSET.

The units.  max: bit-equal.  argmax: the first index of the maximum.  lse, loss: |got - ref| <= C (1 + |ref|).
gradient, element-wise: |got - ref| <= C_G |w gs| (p64 + eps / V + [c == t]) -- a dropped eps / V or a one-hot one lane
off in a class of small probability fails it; where p64 == 0 and eps == 0 the gradient is exactly zero.  partial[g] and
the bias gradient: the same unit summed over the rows that enter the sum."""
from functools import lru_cache
from typing import NamedTuple, Optional, Tuple

import numpy as np

from oracle.nm_oracle import gumbel_noise

PAD = np.float32(3e38)
INT_MAX = 2 ** 31 - 1

# measured on the CPU restatement over the whole table (test_row_cases_ref.py::test_measured_errors_and_the_constants)
E_LSE = 2.321e-7           # |lse32 - lse64| / (1 + |lse64|), row statistics
E_LOSS = 1.502e-7          # |loss32 - loss64| / (1 + |loss64|), every case but the class below
E_G = 1.223e-6             # |g32 - g64| / unit, element-wise, nm_xent and nm_xent_colsum (exp(x - max) at x - max near
#                            -18 carries most of it: the last bits of the argument reduction, relative to the value)
E_P = 1.160e-6             # partial column sums / their unit
E_B = 1.087e-6             # the bias gradient (the sum of the partials) / its unit
C_LSE = 1.0e-6             # 4.3 x E_LSE: ten times would pass the 1e-6 of test_row_stats_and_argmax_ties; the ceiling holds
C_LOSS = 1.5e-6            # 10.0 x E_LOSS
C_G = 1.0e-5               # 8.2 x E_G: the ceiling (test_xent_fwd_and_grad's 1e-5), not ten times
C_P = 1.0e-5               # 8.6 x E_P: the ceiling
C_B = 1.0e-5               # 9.2 x E_B: the ceiling
# Label smoothing with logits near +-1e4: the smoothed term is (max + lse) - sum(x) / V, and a float32 sum of V logits
# of size 1e4 carries an error of some 1e-4 of a logit whoever adds them up -- the restatement itself is beyond the
# 1e-5 ceiling there (E_LOSS_OFFSET), so these cases (content plus1e4 / minus1e4 with eps > 0) have their own measured
# constant; every other case, the same logits without smoothing included, stays on C_LOSS.
E_LOSS_OFFSET = 1.944e-5
C_LOSS_OFFSET = 1.9e-4     # 9.8 x E_LOSS_OFFSET


# ------------------------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------------------------
class Layout(NamedTuple):
    v: int
    ldx: int
    off: int                 # the view starts ``off`` floats into the (aligned) buffer

    @property
    def aligned(self):
        return self.off % 4 == 0


VARIANTS = ("plain", "ld1", "shift", "ld4")


def layout(v: int, variant: str) -> Layout:
    return {"plain": Layout(v, v, 0), "ld1": Layout(v, v + 1, 0), "shift": Layout(v, v, 1),
            "ld4": Layout(v, v + 4, 0)}[variant]


def new_buffer(rows: int, lay: Layout) -> np.ndarray:
    return np.full(lay.off + rows * lay.ldx + 4, PAD, np.float32)


def view(flat: np.ndarray, rows: int, lay: Layout) -> np.ndarray:
    return flat[lay.off:lay.off + rows * lay.ldx].reshape(rows, lay.ldx)[:, :lay.v]


def padding(rows: int, lay: Layout) -> np.ndarray:
    """bool mask over the flat buffer: what is not part of the view."""
    mask = np.ones(lay.off + rows * lay.ldx + 4, bool)
    view(mask, rows, lay)[:] = False
    return mask


# ------------------------------------------------------------------------------------------------------------------
# the three dispatch rules of csrc/nm_logits.hip, restated: functions of V, ldx and alignment only
# ------------------------------------------------------------------------------------------------------------------
SCAN_BRANCHES = ("scan8", "scan16", "scan32", "scalar:V%4", "scalar:ldx%4", "scalar:base", "scalar:V>131072")
XENT_BRANCHES = ("regs8", "regs16", "scalar:V%4", "scalar:ldx%4", "scalar:base", "scalar:V>65536")
COLS_BRANCHES = ("cols2", "cols4", "cols8", "refuse:G<1", "refuse:G>rows", "refuse:V%4", "refuse:ldx%4",
                 "refuse:base", "refuse:partial", "refuse:V>32768")


def row_scan_nv(v: int, ldx: int, aligned: bool) -> str:
    """nm_row_stats: row_scan_kernel<4, NV, false> by V / 4 <= 8192 | 16384 | 32768, row_stats_kernel otherwise."""
    if v % 4:
        return "scalar:V%4"
    if ldx % 4:
        return "scalar:ldx%4"
    if not aligned:
        return "scalar:base"
    v4 = v // 4
    return "scan8" if v4 <= 8192 else "scan16" if v4 <= 16384 else "scan32" if v4 <= 32768 else "scalar:V>131072"


def xent_nv(v: int, ldx: int, aligned: bool) -> str:
    """nm_xent: xent_regs_kernel<8 | 16> by V / 4 <= 8192 | 16384, xent_kernel otherwise."""
    if v % 4:
        return "scalar:V%4"
    if ldx % 4:
        return "scalar:ldx%4"
    if not aligned:
        return "scalar:base"
    v4 = v // 4
    return "regs8" if v4 <= 8192 else "regs16" if v4 <= 16384 else "scalar:V>65536"


def colsum_nv(v: int, ldx: int, aligned: bool, partial_aligned: bool, rows: int, g: int) -> str:
    """nm_xent_colsum: xent_cols_kernel<2 | 4 | 8> by ceil(V / 4 / 1024) <= 2 | 4 | 8, or one of its refusals."""
    if g < 1:
        return "refuse:G<1"
    if g > rows:
        return "refuse:G>rows"
    if v % 4:
        return "refuse:V%4"
    if ldx % 4:
        return "refuse:ldx%4"
    if not aligned:
        return "refuse:base"
    if not partial_aligned:
        return "refuse:partial"
    if v > 32768:
        return "refuse:V>32768"
    nv = (v // 4 + 1023) // 1024
    return "cols2" if nv <= 2 else "cols4" if nv <= 4 else "cols8"


# ------------------------------------------------------------------------------------------------------------------
# references (float64) and restatements (float32, only to measure the tolerances)
# ------------------------------------------------------------------------------------------------------------------
def ref_stats(x):
    """max (of the float32 values), first argmax, lse = log(sum(exp(x - max))) in float64."""
    x64 = x.astype(np.float64)
    m = x64.max(1)
    return x.max(1), x.argmax(1).astype(np.int32), np.log(np.exp(x64 - m[:, None]).sum(1))


def f32_stats(x):
    m = x.max(1)
    return m, x.argmax(1).astype(np.int32), np.log(np.exp(x - m[:, None]).sum(1, dtype=np.float32))


class XentRef(NamedTuple):
    loss: np.ndarray         # [rows] float64
    grad: np.ndarray         # [rows, V] float64
    unit: np.ndarray         # [rows, V] float64: |w gs| (p + eps / V + [c == t])


def _onehot(t, rows, v):
    hot = np.zeros((rows, v), bool)
    inside = (t >= 0) & (t < v)
    hot[np.nonzero(inside)[0], t[inside]] = True
    return hot, inside


def ref_xent(x, t, w, gs, eps) -> XentRef:
    """loss = ((1 - eps) nll + eps (-mean log p)) w with nll = 0 for a target outside [0, V) (TF's one_hot of an
    out-of-range index); gradient = (p - eps / V - (1 - eps) onehot) w gs.  ``w`` None = 1, ``gs`` None = 1."""
    rows, v = x.shape
    x64 = x.astype(np.float64)
    w64 = np.ones(rows) if w is None else w.astype(np.float64)
    gs64 = 1.0 if gs is None else float(gs)
    eps = float(np.float32(eps))
    m = x64.max(1, keepdims=True)
    e = np.exp(x64 - m)
    s = e.sum(1, keepdims=True)
    p = e / s
    hot, inside = _onehot(t, rows, v)
    logp = (x64 - m) - np.log(s)
    nll = np.where(inside, -logp[np.arange(rows), np.clip(t, 0, v - 1)], 0.0)
    loss = (1.0 - eps) * nll
    if eps:
        loss = loss + eps * -logp.mean(1)
    grad = (p - eps / v - (1.0 - eps) * hot) * (w64 * gs64)[:, None]
    unit = np.abs(w64 * gs64)[:, None] * (p + eps / v + hot)
    return XentRef(loss * w64, grad, unit)


def f32_xent(x, t, w, gs, eps):
    """The kernels' arithmetic in float32 numpy: one maximum, exp(x - max), their sum, its reciprocal."""
    f = np.float32
    rows, v = x.shape
    w32 = np.ones(rows, f) if w is None else w
    gs32 = f(1.0) if gs is None else f(gs)
    eps = f(eps)
    bv = x.max(1)
    ex = np.exp(x - bv[:, None])
    s = ex.sum(1, dtype=f)
    lse = np.log(s)
    hot, inside = _onehot(t, rows, v)
    xt = x[np.arange(rows), np.clip(t, 0, v - 1)]
    nll = np.where(inside, -((xt - bv) - lse), f(0.0)).astype(f)
    if eps:
        uniform = (bv + lse) - x.sum(1, dtype=f) / f(v)
        loss = ((f(1.0) - eps) * nll + eps * uniform) * w32
    else:
        loss = nll * w32
    g = ((ex * (f(1.0) / s)[:, None] - eps / f(v)) - (f(1.0) - eps) * hot.astype(f)) * (w32 * gs32)[:, None]
    assert loss.dtype == f and g.dtype == f
    return loss, g


def ref_colsum(ref: XentRef, g: int):
    """partial[j] = the sum of gradient rows j, j + g, ...; its unit; the bias gradient and its unit."""
    part = np.stack([ref.grad[j::g].sum(0) for j in range(g)])
    unit = np.stack([ref.unit[j::g].sum(0) for j in range(g)])
    return part, unit, ref.grad.sum(0), ref.unit.sum(0)


def f32_colsum(grad32, g: int):
    part = np.zeros((g, grad32.shape[1]), np.float32)
    for r in range(grad32.shape[0]):                     # the accumulator of a workgroup takes its rows in order
        part[r % g] += grad32[r]
    return part, part.sum(0, dtype=np.float32)


def gumbel_u(rows: int, vocab: int, salt: int) -> np.ndarray:
    """The uniforms behind oracle.nm_oracle.gumbel_noise, exactly, as float64 (23 bits + 0.5 over 2^23)."""
    def mix(x):
        x = x.astype(np.uint32)
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x21F0AAAD)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x735A2D97)
        x ^= x >> np.uint32(15)
        return x
    with np.errstate(over="ignore"):
        key = mix(np.uint32(salt & 0xFFFFFFFF) + np.arange(rows, dtype=np.uint32) * np.uint32(0x85EBCA6B))
        bits = mix(np.arange(vocab, dtype=np.uint32)[None, :] * np.uint32(0x9E3779B1) + key[:, None])
    return ((bits >> np.uint32(9)).astype(np.float64) + 0.5) / 8388608.0


def ref_draw(x, salt):
    """argmax(x + g) with the noise in float64."""
    return (x.astype(np.float64) - np.log(-np.log(gumbel_u(x.shape[0], x.shape[1], salt)))).argmax(1)


def f32_draw(x, salt):
    """argmax(x + O.gumbel_noise(...)) in float32, with the noisy logits."""
    noisy = x + gumbel_noise(x.shape[0], x.shape[1], salt)
    return noisy.argmax(1), noisy


# ------------------------------------------------------------------------------------------------------------------
# row statistics
# ------------------------------------------------------------------------------------------------------------------
STATS_V = (1, 3, 4, 5, 63, 64, 65, 1023, 1024, 4096, 4100, 32001, 32768, 32772, 65536, 65540, 131072, 131076)
STATS_GROUPS = ("values", "maxpos", "ties")
TIE_THREAD = (3, 4099)       # c and c + 4096: two columns of one thread in both kernels
TIE_LANES = (8, 12)          # two lanes of one wave (threads 2 and 3 of the vector kernel, 8 and 12 of the scalar one)
TIE_WAVES = (8, 264)         # two waves (threads 2 and 66 of the vector kernel, 8 and 264 of the scalar one)


class StatsCase(NamedTuple):
    name: str
    v: int
    variant: str
    group: str
    seed: int


def stats_kinds(v: int, group: str):
    """The rows of a case: one of each content the size allows."""
    if group == "values":
        return ["normal", "plus1e4", "minus1e4", "all_equal", "quarter_ninf", "one_finite"]
    if group == "maxpos":
        return ["max_last"] + (["max_lane0", "max_lane1", "max_lane2", "max_lane3"] if v >= 4 else [])
    kinds = []
    if v > TIE_THREAD[1]:
        kinds.append("tie_thread")
    if v > TIE_LANES[1]:
        kinds.append("tie_lanes")
    if v > TIE_WAVES[1]:
        kinds.append("tie_waves")
    if v >= 2:
        kinds.append("tie_first_last")
    return kinds


def _variants(v):
    return VARIANTS if v % 4 == 0 else ("plain",)


def _stats_cases():
    out = []
    for v in STATS_V:
        for variant in _variants(v):
            for group in STATS_GROUPS:
                if stats_kinds(v, group):
                    out.append(StatsCase("s_v{}_{}_{}".format(v, variant, group), v, variant, group, 1000 + len(out)))
    return out


STATS_CASES = _stats_cases()
STATS_BY_NAME = {c.name: c for c in STATS_CASES}


class StatsBuilt(NamedTuple):
    case: StatsCase
    lay: Layout
    kinds: list
    flat: np.ndarray         # the whole buffer, padding included
    x: np.ndarray            # its [rows, V] view
    max: np.ndarray
    argmax: np.ndarray
    lse: np.ndarray          # float64
    pinned: dict             # row -> the one admissible argmax of a tie / degenerate row


def _stats_row(kind, v, rng, pinned, r):
    x = (rng.randn(v) * 3).astype(np.float32)
    top = np.float32(x.max() + np.float32(1.5))
    if kind == "plus1e4":
        x += np.float32(1e4)
    elif kind == "minus1e4":
        x -= np.float32(1e4)
    elif kind == "all_equal":
        x[:] = 1.0
        pinned[r] = 0
    elif kind == "quarter_ninf":
        x[rng.choice(v, v // 4, replace=False)] = -np.inf
    elif kind == "one_finite":
        keep = int(rng.randint(v))
        value = x[keep]
        x[:] = -np.inf
        x[keep] = value
        pinned[r] = keep
    elif kind == "max_last":
        x[v - 1] = top
        pinned[r] = v - 1
    elif kind.startswith("max_lane"):
        col = v - 4 + int(kind[-1])                      # the four lanes of the last float4 (V % 4 == 0)
        x[col] = top
        pinned[r] = col
    elif kind.startswith("tie_"):
        a, b = {"tie_thread": TIE_THREAD, "tie_lanes": TIE_LANES, "tie_waves": TIE_WAVES,
                "tie_first_last": (0, v - 1)}[kind]
        x[a] = x[b] = top
        pinned[r] = a
    return x


@lru_cache(maxsize=4)
def build_stats(name: str) -> StatsBuilt:
    """Inputs and float64 reference of a case: computed once, shared, never written to."""
    c = STATS_BY_NAME[name]
    lay = layout(c.v, c.variant)
    kinds = stats_kinds(c.v, c.group)
    rng = np.random.RandomState(c.seed)
    flat = new_buffer(len(kinds), lay)
    x = view(flat, len(kinds), lay)
    pinned = {}
    for r, kind in enumerate(kinds):
        x[r] = _stats_row(kind, c.v, rng, pinned, r)
    flat.setflags(write=False)
    mx, am, lse = ref_stats(x)
    return StatsBuilt(c, lay, kinds, flat, x, mx, am, lse, pinned)


# every subset of the three optional outputs, at one vector and one scalar size
SUBSET_CASES = ("s_v4096_plain_values", "s_v4100_ld1_values")
# the degenerate rows (all -inf, all NaN, NaN in every other column) beside an ordinary row
DEGENERATE_LAYOUTS = ((1024, "plain"), (1023, "plain"))


def degenerate_rows(v: int, seed: int = 7):
    """[4, V]: an ordinary row, all -inf, all NaN, NaN in every other column; the argmax each must give (np.argmax
    for the all -inf row: the first index; the first maximum of the other columns beside NaN) or None = any of [0, V)."""
    x = (np.random.RandomState(seed).randn(4, v) * 3).astype(np.float32)
    x[1] = -np.inf
    x[2] = np.nan
    x[3, ::2] = np.nan
    want = [int(x[0].argmax()), 0, None, int(np.nanargmax(x[3]))]
    return x, want


# ------------------------------------------------------------------------------------------------------------------
# cross entropy
# ------------------------------------------------------------------------------------------------------------------
XENT_V = (1, 4, 37, 40, 4096, 4100, 32768, 32772, 65536, 65540, 65541)
XENT_CONTENT_LAYOUTS = ((4096, "plain"), (40, "ld1"), (32772, "plain"), (65536, "plain"), (65541, "plain"))
XENT_OPTION_LAYOUTS = ((4100, "plain"), (65541, "plain"))
GRAD_SCALE = np.float32(0.37)


class XentCase(NamedTuple):
    name: str
    v: int
    variant: str
    eps: float
    targets: str             # "in" | "edge"
    content: str             # "normal" | "plus1e4" | "minus1e4" | "ninf"
    options: Tuple[bool, bool, bool]   # weights given, grad_scale given, loss_rows given
    seed: int


def xent_targets(v: int, group: str):
    if group == "in":
        mid = 4 * (v // 8)
        seen = []
        for t in (0, v - 1, mid, mid + 1, mid + 2, mid + 3):      # the ends and each float4 lane
            if 0 <= t < v and t not in seen:
                seen.append(t)
        return seen
    return [t for t in (4095, 4096, 4097) if t < v] + [-1, v, INT_MAX]


def _xent_cases():
    out = []

    def add(v, variant, eps, tg, content="normal", options=(True, True, True)):
        name = "x_v{}_{}_eps{}_{}_{}".format(v, variant, "01" if eps else "0", tg, content)
        if options != (True, True, True):
            name += "_" + "".join(k if on else "-" for k, on in zip("wgl", options))
        out.append(XentCase(name, v, variant, eps, tg, content, options, 2000 + len(out)))

    for v in XENT_V:
        for variant in _variants(v):
            for eps in (0.0, 0.1):
                for tg in ("in", "edge"):
                    add(v, variant, eps, tg)
    for v, variant in XENT_CONTENT_LAYOUTS:
        for content in ("plus1e4", "minus1e4"):
            for eps in (0.0, 0.1):
                add(v, variant, eps, "in", content)
        add(v, variant, 0.0, "in", "ninf")
    for v, variant in XENT_OPTION_LAYOUTS:
        for k in range(7):                                # the eighth combination is the table's default
            add(v, variant, 0.1, "in", options=(bool(k & 1), bool(k & 2), bool(k & 4)))
    return out


XENT_CASES = _xent_cases()
XENT_BY_NAME = {c.name: c for c in XENT_CASES}


class XentBuilt(NamedTuple):
    case: object
    lay: Layout
    rows: int
    flat: np.ndarray
    x: np.ndarray
    targets: np.ndarray      # int32
    weights: Optional[np.ndarray]
    grad_scale: Optional[np.float32]
    ref: XentRef
    offset_class: bool       # on C_LOSS_OFFSET instead of C_LOSS


def _row_weights(rows, rng, seed):
    """uniform(0.5, 1.5) with one zero and one negative weight (REINFORCE and self-critical rewards are signed)."""
    w = rng.uniform(0.5, 1.5, rows).astype(np.float32)
    if rows >= 2:
        w[seed % rows] = 0.0
    if rows >= 3:
        w[(seed + 1) % rows] *= np.float32(-1.0)
    return w


def _xent_logits(x, targets, content, rng):
    rows, v = x.shape
    x[:] = (rng.randn(rows, v) * 2).astype(np.float32)
    if content == "plus1e4":
        x += np.float32(1e4)
    elif content == "minus1e4":
        x -= np.float32(1e4)
    elif content == "ninf":
        for r in range(rows):                             # a quarter of the classes masked, never the target
            masked = rng.choice(v, v // 4, replace=False)
            x[r, masked[masked != targets[r]]] = -np.inf
            x[r, 0 if targets[r] != 0 else 1] = -np.inf   # thread 0 of every kernel holds a masked class


@lru_cache(maxsize=4)
def build_xent(name: str) -> XentBuilt:
    c = XENT_BY_NAME[name]
    lay = layout(c.v, c.variant)
    rng = np.random.RandomState(c.seed)
    targets = np.array(xent_targets(c.v, c.targets), np.int32)
    rows = len(targets)
    flat = new_buffer(rows, lay)
    x = view(flat, rows, lay)
    _xent_logits(x, targets, c.content, rng)
    weights = _row_weights(rows, rng, c.seed) if c.options[0] else None
    gs = GRAD_SCALE if c.options[1] else None
    for a in (flat, targets) + (() if weights is None else (weights,)):
        a.setflags(write=False)
    ref = ref_xent(x, targets, weights, gs, c.eps)
    return XentBuilt(c, lay, rows, flat, x, targets, weights, gs, ref,
                     c.content in ("plus1e4", "minus1e4") and c.eps > 0)


# ------------------------------------------------------------------------------------------------------------------
# cross entropy with column sums
# ------------------------------------------------------------------------------------------------------------------
COLS_V = (4, 8, 1024, 8192, 8196, 16384, 16388, 32768)
COLS_ROWS_G = ((1, 1), (2, 2), (7, 1), (7, 3), (7, 7), (5, 4))


class ColsCase(NamedTuple):
    name: str
    v: int
    variant: str             # "plain" | "ld4"
    rows: int
    g: int
    eps: float
    content: str
    seed: int


def _cols_cases():
    out = []
    for v in COLS_V:
        for rows, g in COLS_ROWS_G:
            for variant in ("plain", "ld4"):
                for eps in (0.0, 0.1):
                    out.append(ColsCase("c_v{}_{}_r{}_g{}_eps{}".format(v, variant, rows, g, "01" if eps else "0"),
                                        v, variant, rows, g, eps, "normal", 3000 + len(out)))
    for v in (1024, 32768):                               # masked classes through the column kernel as well
        out.append(ColsCase("c_v{}_plain_r5_g4_eps0_ninf".format(v), v, "plain", 5, 4, 0.0, "ninf", 3000 + len(out)))
    return out


COLS_CASES = _cols_cases()
COLS_BY_NAME = {c.name: c for c in COLS_CASES}


def cols_targets(v: int, rows: int, seed: int):
    """``rows`` targets out of the ends, the float4 lanes and the three kinds outside [0, V), rotated by the seed."""
    mid = 4 * (v // 8)
    pool = [v - 1, -1, 0, mid + 1, v, mid + 2, INT_MAX, mid, mid + 3]
    return [pool[(seed + r) % len(pool)] for r in range(rows)]


@lru_cache(maxsize=4)
def build_cols(name: str) -> XentBuilt:
    c = COLS_BY_NAME[name]
    lay = layout(c.v, c.variant)
    rng = np.random.RandomState(c.seed)
    targets = np.array(cols_targets(c.v, c.rows, c.seed), np.int32)
    flat = new_buffer(c.rows, lay)
    x = view(flat, c.rows, lay)
    _xent_logits(x, targets, c.content, rng)
    weights = _row_weights(c.rows, rng, c.seed)
    for a in (flat, targets, weights):
        a.setflags(write=False)
    return XentBuilt(c, lay, c.rows, flat, x, targets, weights, GRAD_SCALE,
                     ref_xent(x, targets, weights, GRAD_SCALE, c.eps), False)


# (what, V, ldx - V, view offset, partial offset, rows, G): host checks, nothing is launched
COLS_REFUSALS = (
    ("V%4", 1022, 2, 0, 0, 3, 1),
    ("V=32772", 32772, 0, 0, 0, 3, 1),
    ("G=0", 1024, 0, 0, 0, 3, 0),
    ("G>rows", 1024, 0, 0, 0, 3, 4),
    ("partial off alignment", 1024, 0, 0, 1, 3, 1),
    ("ldx%4", 1024, 2, 0, 0, 3, 1),
    ("logits off alignment", 1024, 0, 1, 0, 3, 1),
)


# ------------------------------------------------------------------------------------------------------------------
# the draw
# ------------------------------------------------------------------------------------------------------------------
DRAW_SALTS = (0, 12345, 0xFFFFFFFF)
DRAW_GAP = 1e-4              # the rule of tests/test_sampling_gpu.py


class DrawCase(NamedTuple):
    name: str
    rows: int
    v: int
    pad: int
    seed: int                # chosen (asserted by the CPU test): under every salt the restated draw of every row wins
    #                          by more than DRAW_GAP and equals the float64 draw, so the rule pins one symbol per row


DRAW_CASES = [
    DrawCase("d_r1_v1", 1, 1, 0, 1),
    DrawCase("d_r5_v1_pad3", 5, 1, 3, 2),
    DrawCase("d_r7_v255", 7, 255, 0, 3),
    DrawCase("d_r7_v256_pad4", 7, 256, 4, 4),
    DrawCase("d_r7_v257_pad3", 7, 257, 3, 5),
    DrawCase("d_r3_v32001_pad1", 3, 32001, 1, 6),
]
DRAW_BY_NAME = {c.name: c for c in DRAW_CASES}


@lru_cache(maxsize=None)
def build_draw(name: str):
    """(layout, flat buffer, view)."""
    c = DRAW_BY_NAME[name]
    lay = Layout(c.v, c.v + c.pad, 0)
    flat = new_buffer(c.rows, lay)
    x = view(flat, c.rows, lay)
    x[:] = (np.random.RandomState(c.seed).randn(c.rows, c.v) * 2).astype(np.float32)
    flat.setflags(write=False)
    return lay, flat, x


# ------------------------------------------------------------------------------------------------------------------
# the errors of the float32 restatement (what E_* record) and the checks both test files share
# ------------------------------------------------------------------------------------------------------------------
def scaled(got, ref):
    """max |got - ref| / (1 + |ref|)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (1.0 + np.abs(ref))).max()) if ref.size else 0.0


def in_units(got, ref, unit):
    """max |got - ref| / unit over the elements with a unit; where the unit is 0, ``got`` must be exactly 0."""
    got = np.asarray(got, np.float64)
    live = unit > 0
    assert (got[~live] == 0).all(), "a gradient whose unit is zero must be exactly zero"
    return float((np.abs(got - ref)[live] / unit[live]).max()) if live.any() else 0.0


def loss_bound(b: XentBuilt) -> float:
    return C_LOSS_OFFSET if b.offset_class else C_LOSS
