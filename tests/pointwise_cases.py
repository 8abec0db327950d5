"""Seeded inputs, expected values and bounds of the point-wise kernel tests, shared by the GPU tests
(tests/test_pointwise_kernels_gpu.py: kernel against the float64 evaluation) and the CPU tests
(tests/test_pointwise_refs.py: the float32 evaluation of the same reference on the same inputs stays inside the same
bound -- the bound can be met by plain fp32 arithmetic on inputs of that size).

A family is (cases, inputs(case) -> dict of float32 / int32 arrays, expect(case, inputs, dtype) -> dict of arrays, and
the bound of each output).  Inputs are cached: the production-size arrays are built once per process."""
import functools

import numpy as np
import torch

from oracle import pointwise_ref as P

# ---- bounds (absolute, times max(1, |ref|max)) ---------------------------------------------------------------------
TOL_ACT = 1e-6       # one activation / a couple of fp32 operations: the bound of test_elementwise_primitives
TOL_FUSED = 2e-5     # fused cells, their backwards, the softmax pair, layer_norm_bwd: the bound of the layer-norm tests


def bound(tol, ref):
    ref = np.asarray(ref, dtype=np.float64)
    fin = ref[np.isfinite(ref)]
    return tol * max(1.0, float(np.abs(fin).max()) if fin.size else 1.0)


def sum_bound(n_addends, scale):
    """A float32 sum of n terms of magnitude ``scale`` in some order: the bound of test_colsum_both_kernels."""
    return 2e-6 * np.sqrt(max(n_addends, 1)) * max(1.0, scale)


def max_err(got, ref):
    """max |got - ref| over the finite reference entries; non-finite entries (-inf) must be equal."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    if not np.array_equal(got[~fin], ref[~fin]):
        return float("inf")
    return float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0


def np64(t):
    return t.detach().numpy().astype(np.float64) if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def _seed(name):
    """A stable integer of a name (hash() of a str changes from process to process)."""
    import zlib
    return zlib.crc32(name.encode())


def normal(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


# shapes [rows, cols]: tiny and odd; mid with ragged tails; past the first trip of a 4096 x 256 grid-stride loop
TINY, MID, LONG = (3, 5), (301, 131), (1031, 1021)
PW_SHAPES = (TINY, MID, LONG)
# nm_ew: [6400, 1536] contiguous is 2 457 600 float4 (second trip of the float4 kernel starts at 1 048 576);
# 1535 of 1536 columns forces the scalar kernel at the same size
EW_SHAPES = (TINY, MID, (6400, 1536), (6400, 1535))
EW_ALPHA = {"scale": 0.37, "sigmoid": 0.75, "add_scalar": -1.25}


# ---- nm_ew ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _ew_base(shape):
    rng = np.random.default_rng([_seed("ew"), shape[0], shape[1]])
    return normal(rng, shape), normal(rng, shape), normal(rng, shape)


def ew_inputs(op, shape):
    """(a, b or None, base): ``base`` is what an accumulating call finds in the output."""
    n0, n1, base = _ew_base(shape)
    a, b = n0, (n1 if op in P.EW_BINARY else None)
    flat = np.arange(a.size).reshape(shape)
    if op in ("sigmoid", "tanh"):
        # |x| of 30 .. 100 on every 7th element: exp overflows in fp32 at 88.7, the result must saturate
        big = (30.0 + 70.0 * ((flat % 97) / 96.0)) * np.where(flat % 2 == 0, 1.0, -1.0)
        a = np.where(flat % 7 == 0, big, a * 3.0).astype(np.float32)
    elif op == "sigmoid_bwd":
        a = (1.0 / (1.0 + np.exp(-n0.astype(np.float64) * 3.0))).astype(np.float32)
    elif op == "tanh_bwd":
        a = np.tanh(n0.astype(np.float64) * 2.0).astype(np.float32)
    elif op == "relu_bwd":
        a = np.maximum(n0, 0.0)
    elif op == "logaddexp":
        a, b = (n0 * 5.0).astype(np.float32), (n1 * 5.0).astype(np.float32)
        k = flat % 11
        a = np.where(k == 0, -np.inf, a)                        # -inf on one side
        a, b = np.where(k == 1, -np.inf, a), np.where(k == 1, -np.inf, b)      # ... on both: -inf, not NaN
        b = np.where(k == 2, a, b)                              # equal arguments
        a, b = np.where(k == 3, 80.0, a), np.where(k == 3, -75.0, b)           # widely separated
        b = np.where(k == 4, -np.inf, b)
        a, b = a.astype(np.float32), b.astype(np.float32)
    elif op == "div":
        b = (np.sign(n1) * (0.5 + np.abs(n1))).astype(np.float32)
        b[b == 0] = 0.5
    elif op == "rowscale":
        b = np.ascontiguousarray(n1[:, :1])
    return a, b, base


def ew_expect(op, a, b, dtype):
    return P.ew(op, a.astype(dtype), None if b is None else b.astype(dtype), EW_ALPHA.get(op, 0.0))


def ew_tol(op):
    return 0.0 if op in P.EW_EXACT else TOL_ACT


# ---- cells ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def lstm_inputs(rows, h):
    rng = np.random.default_rng([_seed("lstm"), rows, h])
    z = normal(rng, (rows, 4 * h), 2.0)
    flat = np.arange(z.size).reshape(z.shape)
    z = np.where(flat % 11 == 0, np.where(flat % 2 == 0, 20.0, -20.0), z).astype(np.float32)      # saturated gates
    return dict(z=z, c_prev=normal(rng, (rows, h)), dh=normal(rng, (rows, h)), dc_new=normal(rng, (rows, h)),
                base_dz=normal(rng, (rows, 4 * h)), base_dc=normal(rng, (rows, h)))


def lstm_expect(inp, forget_bias, dtype, use_dh=True, use_dc=True):
    td = torch.float64 if dtype == np.float64 else torch.float32
    z, c_prev = torch.tensor(inp["z"], dtype=td), torch.tensor(inp["c_prev"], dtype=td)
    c_new, h_new, gates = P.lstm_cell(z, c_prev, forget_bias)
    dz, dc_prev = P.lstm_cell_grads(z, c_prev, forget_bias, torch.tensor(inp["dh"], dtype=td) if use_dh else None,
                                    torch.tensor(inp["dc_new"], dtype=td) if use_dc else None)
    return dict(c_new=c_new, h_new=h_new, gates=gates, dz=dz, dc_prev=dc_prev)


@functools.lru_cache(maxsize=8)
def nematus_inputs(rows, h):
    rng = np.random.default_rng([_seed("nematus"), rows, h])
    return dict(g_pre=normal(rng, (rows, 2 * h), 1.5), g2=normal(rng, (rows, 2 * h)), sc=normal(rng, (rows, h)),
                ci=normal(rng, (rows, h)), h_prev=normal(rng, (rows, h)), dh=normal(rng, (rows, h)),
                base_dg=normal(rng, (rows, 2 * h)), base_dci=normal(rng, (rows, h)), base_dsc=normal(rng, (rows, h)),
                base_dhp=normal(rng, (rows, h)))


def nematus_expect(inp, with_g2, dtype):
    td = torch.float64 if dtype == np.float64 else torch.float32
    t = {k: torch.tensor(v, dtype=td) for k, v in inp.items()}
    g2 = t["g2"] if with_g2 else None
    h_new, ru, c = P.nematus_cell(t["g_pre"], t["sc"], t["ci"], t["h_prev"], g2)
    dg, dci, dsc, dhp = P.nematus_cell_grads(t["g_pre"], t["sc"], t["ci"], t["h_prev"], t["dh"], g2)
    return dict(h_new=h_new, ru=ru, c=c, dg=dg, dci=dci, dsc=dsc, dh_prev=dhp)


@functools.lru_cache(maxsize=8)
def blend_inputs(rows, cols):
    rng = np.random.default_rng([_seed("blend"), rows, cols])
    u = (1.0 / (1.0 + np.exp(-rng.standard_normal((rows, cols)) * 2.0))).astype(np.float32)
    return dict(u=u, h=normal(rng, (rows, cols)), c=normal(rng, (rows, cols)), dy=normal(rng, (rows, cols)),
                base_du=normal(rng, (rows, cols)), base_dh=normal(rng, (rows, cols)), base_dc=normal(rng, (rows, cols)))


def blend_expect(inp, dtype):
    td = torch.float64 if dtype == np.float64 else torch.float32
    t = {k: torch.tensor(v, dtype=td) for k, v in inp.items()}
    du, dh, dc = P.blend_grads(t["dy"], t["u"], t["h"], t["c"])
    return dict(out=P.blend(t["u"], t["h"], t["c"]), du=du, dh=dh, dc=dc)


SELECT_T = 3


@functools.lru_cache(maxsize=8)
def select_inputs(rows, cols):
    rng = np.random.default_rng([_seed("select"), rows, cols])
    # lengths 0, t, t + 1 and one past the last step, in turn
    lengths = np.array([(0, SELECT_T, SELECT_T + 1, 1000)[r % 4] for r in range(rows)], dtype=np.int32)
    return dict(h_new=normal(rng, (rows, cols)), h_prev=normal(rng, (rows, cols)), dh=normal(rng, (rows, cols)),
                dy=normal(rng, (rows, cols)), base_new=normal(rng, (rows, cols)), base_prev=normal(rng, (rows, cols)),
                lengths=lengths)


def select_expect(inp, dtype, lengths=True, use_dh=True, use_dy=True):
    td = torch.float64 if dtype == np.float64 else torch.float32
    t = {k: torch.tensor(v, dtype=td) for k, v in inp.items() if k != "lengths"}
    ln = inp["lengths"] if lengths else None
    h_out, y_out = P.rnn_select(t["h_new"], t["h_prev"], ln, SELECT_T)
    d_new, d_prev = P.rnn_select_grads(t["h_new"], t["h_prev"], ln, SELECT_T, t["dh"] if use_dh else None,
                                       t["dy"] if use_dy else None)
    return dict(h_out=h_out, y_out=y_out, d_new=d_new, d_prev=d_prev)


# ---- tanh_bwd ------------------------------------------------------------------------------------------------------
TANH_BWD_N = (1, 3, 7, 1023, 1025, 1048579)        # n < 4, scalar tails, and past 2^20


@functools.lru_cache(maxsize=8)
def tanh_bwd_inputs(n):
    rng = np.random.default_rng([_seed("tanh_bwd"), n])
    pre = normal(rng, (n,), 1.5)
    return dict(pre=pre, y=np.tanh(pre.astype(np.float64)).astype(np.float32), dy=normal(rng, (n,)))


def tanh_bwd_expect(inp, dtype):
    td = torch.float64 if dtype == np.float64 else torch.float32
    return P.tanh_grads(torch.tensor(inp["pre"], dtype=td), torch.tensor(inp["dy"], dtype=td))


# ---- layer_norm_bwd ------------------------------------------------------------------------------------------------
LN_SHAPES = ((6400, 512), (37, 512), (640, 2048), (5, 8), (300, 132), (1, 1024), (33, 131))


@functools.lru_cache(maxsize=8)
def ln_inputs(rows, d):
    rng = np.random.default_rng([_seed("ln"), rows, d])
    x = (rng.standard_normal((rows, d)) * 2.0 + 0.5).astype(np.float32)
    return dict(x=x, dy=normal(rng, (rows, d)), gamma=(1.0 + 0.3 * rng.standard_normal(d)).astype(np.float32),
                beta=normal(rng, (d,), 0.1))


def ln_expect(inp, dtype):
    td = torch.float64 if dtype == np.float64 else torch.float32
    t = {k: torch.tensor(v, dtype=td) for k, v in inp.items()}
    _, xhat, mean, rstd = P.layer_norm(t["x"], t["gamma"], t["beta"])
    dx, dgamma, _ = P.layer_norm_grads(t["x"], t["gamma"], t["beta"], t["dy"])
    return dict(dx=dx, dyx=t["dy"] * xhat, dgamma=dgamma, mean=mean, rstd=rstd)


# ---- masked softmax pair -------------------------------------------------------------------------------------------
SOFTMAX_S = (1, 50, 64, 65, 300)        # on either side of the one-wave width
SOFTMAX_B, SOFTMAX_T = 3, 2


@functools.lru_cache(maxsize=16)
def softmax_inputs(s, rpk):
    """T * B * rpk query rows over B sentences whose masks all differ; sentence 1 is fully masked."""
    rng = np.random.default_rng([_seed("softmax"), s, rpk])
    rows = SOFTMAX_T * SOFTMAX_B * rpk
    e = rng.uniform(-40.0, 40.0, (rows, s)).astype(np.float32)
    lens = [s, 0, max(1, (2 * s) // 3)]
    mask = np.zeros((SOFTMAX_B, s), dtype=np.float32)
    for b, ln in enumerate(lens):
        mask[b, :ln] = 1.0
    if s > 2:
        mask[2, 0] = 0.0              # not a prefix: differs from sentence 0 even when 2s/3 rounds to s
    return dict(e=e, mask=mask, dw=normal(rng, (rows, s)))


def softmax_expect(inp, rpk, dtype, masked=True):
    td = torch.float64 if dtype == np.float64 else torch.float32
    e, dw = torch.tensor(inp["e"], dtype=td), torch.tensor(inp["dw"], dtype=td)
    rows = e.shape[0]
    m_fwd = P.mask_rows(torch.tensor(inp["mask"], dtype=td), rows, SOFTMAX_B, rpk) if masked else None
    m_bwd = P.mask_rows(torch.tensor(inp["mask"], dtype=td), rows, SOFTMAX_B, 1) if masked else None
    return dict(w=P.attn_softmax(e, m_fwd), de=P.attn_softmax_grads(e, m_bwd, dw))


# ---- what the CPU suite walks: (label, thunk(dtype) -> {name: array}, {name: tol}) ----------------------------------
def headroom_items():
    for op in P.EW_OPS:
        if ew_tol(op) == 0.0:
            continue
        for shape in EW_SHAPES:
            a, b, _ = ew_inputs(op, shape)
            yield ("ew {} {}".format(op, shape), (lambda dt, op=op, a=a, b=b: {"out": ew_expect(op, a, b, dt)}),
                   {"out": TOL_ACT})
    for rows, h in PW_SHAPES:
        for fb in (0.0, 1.0):
            yield ("lstm {}x{} fb={}".format(rows, h, fb),
                   (lambda dt, rows=rows, h=h, fb=fb: lstm_expect(lstm_inputs(rows, h), fb, dt)),
                   dict.fromkeys(("c_new", "h_new", "gates", "dz", "dc_prev"), TOL_FUSED))
        for g2 in (False, True):
            yield ("nematus {}x{} g2={}".format(rows, h, g2),
                   (lambda dt, rows=rows, h=h, g2=g2: nematus_expect(nematus_inputs(rows, h), g2, dt)),
                   dict.fromkeys(("h_new", "ru", "c", "dg", "dci", "dsc", "dh_prev"), TOL_FUSED))
        yield ("blend {}x{}".format(rows, h), (lambda dt, rows=rows, h=h: blend_expect(blend_inputs(rows, h), dt)),
               dict.fromkeys(("out", "du", "dh", "dc"), TOL_ACT))
        yield ("select {}x{}".format(rows, h), (lambda dt, rows=rows, h=h: select_expect(select_inputs(rows, h), dt)),
               dict.fromkeys(("h_out", "y_out", "d_new", "d_prev"), TOL_ACT))
    for n in TANH_BWD_N:
        yield ("tanh_bwd {}".format(n), (lambda dt, n=n: {"dpre": tanh_bwd_expect(tanh_bwd_inputs(n), dt)}),
               {"dpre": TOL_ACT})
    for rows, d in LN_SHAPES:
        yield ("layer_norm_bwd {}x{}".format(rows, d), (lambda dt, rows=rows, d=d: ln_expect(ln_inputs(rows, d), dt)),
               {"dx": TOL_FUSED, "dyx": TOL_FUSED})
    for s in SOFTMAX_S:
        for rpk in (1, 5):
            yield ("softmax S={} rpk={}".format(s, rpk),
                   (lambda dt, s=s, rpk=rpk: softmax_expect(softmax_inputs(s, rpk), rpk, dt)),
                   {"w": TOL_FUSED, "de": TOL_FUSED})


# ---- inputs of the sum-type and accumulating tests -----------------------------------------------------------------
REDUCE_N = (1, 1000, 65536, 65537, 320000, 4194368)
TIME_SUM_SHAPES = ((3, 1, 5), (7, 50, 33), (64, 50, 512), (1031, 1, 1021), (1031, 2, 1021))
SCATTER_CASES = ((7, 5, 3, 2), (50, 70, 600, 4), (300, 512, 6400, 6), (32000, 100, 2000, 1500))     # V, E, n, hot ids
DROPOUT_SHAPES = PW_SHAPES + ((6400, 1536),)
DROPOUT_SALT, DROPOUT_KEEP = 0x9D2C5680, 0.7


def reduce_inputs(n):
    x = normal(np.random.default_rng(n), (n,))
    x[-1] = 3.0                                     # the last element of the last slice counts
    return x


def time_sum_inputs(b, t, d):
    rng = np.random.default_rng([b, t, d, 5])
    return normal(rng, (b, t, d)), normal(rng, (b, d)), normal(rng, (b, t, d))      # x, dy, base


def scatter_inputs(vocab, e, n, hot):
    """(ids, d, base [V + 2, E]): heavy duplication, id 0 among the ids, three ids outside [0, V)."""
    rng = np.random.default_rng([vocab, e, n])
    ids = rng.integers(0, hot, n).astype(np.int32)
    ids[rng.integers(0, n, max(1, n // 10))] = vocab - 1
    if n >= 10:
        ids[[1, 5, 7]] = (-1, vocab, vocab + 5)                  # out of range: ignored
        ids[[2, 3]] = 0
    return ids, normal(rng, (n, e)), normal(rng, (vocab + 2, e))


def scatter_kept(ids, vocab, skip_pad):
    return (ids >= 0) & (ids < vocab) & ((ids != 0) | (not skip_pad))


def dropout_inputs(rows, cols):
    rng = np.random.default_rng([rows, cols, 77])
    return normal(rng, (rows, cols)), normal(rng, (rows, cols))                      # x, base


# nm_gemm_f32_group: m, n, k, ta, tb, count -- the dispatch boundary from both sides, deep K, a single tile
GROUP_HAND = [
    (512, 512, 640, True, False, 48), (512, 512, 640, True, False, 6), (256, 256, 128, False, False, 47),
    (129, 257, 64, False, True, 48), (4, 4, 4, True, True, 1), (512, 1536, 6400, True, False, 2),
    (132, 68, 1024, True, False, 6), (301, 260, 36, False, False, 2),
] + [case for ta in (False, True) for tb in (False, True)          # both tile dispatches in every layout
     for case in ((256, 256, 128, ta, tb, 48), (132, 68, 64, ta, tb, 2))]


def group_bound(k):
    """Relative to the largest entry of the product: the bound of test_gemm."""
    return 2e-6 * np.sqrt(k) + 1e-6


def group_members(rng, m, n, k, ta, tb, count, pads):
    """``count`` members (a_full, b_full, c0, a, b): the operands inside buffers whose rows are pads[i] floats longer
    (ldc rounded up to a multiple of 4 whatever N is); a is scaled so that the products are O(1)."""
    pad_a, pad_b, pad_c = pads[0], pads[1], pads[2] + (-n) % 4
    scale = 1.0 / np.sqrt(k)
    members = []
    for _ in range(count):
        a_full = (rng.standard_normal((k, m + pad_a) if ta else (m, k + pad_a)) * scale).astype(np.float32)
        b_full = rng.standard_normal((n, k + pad_b) if tb else (k, n + pad_b)).astype(np.float32)
        c0 = rng.standard_normal((m, n + pad_c)).astype(np.float32)
        members.append((a_full, b_full, c0, a_full[:, :m] if ta else a_full[:, :k], b_full[:, :k] if tb else b_full[:, :n]))
    return members


def group_hand_runs(m, n, k, ta, tb, count):
    """The four runs of a hand-picked shape: (pads, accumulate, members)."""
    rng = np.random.default_rng([m, n, k, count])
    for pads in ((0, 0, 0), (4, 8, 4)):
        for acc in (False, True):
            yield pads, acc, group_members(rng, m, n, k, ta, tb, count, pads)


def group_sweep_runs():
    """The seeded sweep: (label, (m, n, k, ta, tb, count), pads, accumulate, members)."""
    rng = np.random.default_rng(20261016)
    free = [1, 3, 5, 17, 33, 63, 65, 100, 127, 129, 200, 260, 301, 512]
    mult4 = [4, 8, 12, 16, 36, 64, 68, 100, 128, 132, 200, 256, 260, 384, 512]
    for case in range(40):
        ta, tb = bool(rng.integers(2)), bool(rng.integers(2))
        m = int(rng.choice(mult4 if ta else free))               # M is contiguous in a transposed A
        n = int(rng.choice(free if tb else mult4))               # N is contiguous in a B that is not transposed
        k = int(rng.choice(free + [1024] if (ta and not tb) else mult4 + [1024]))      # K: contiguous unless A^T and B
        count = int(rng.choice([1, 2, 6, 48]))
        if count == 48 and m * n * k > 256 * 256 * 256:
            count = 6
        pads = tuple(int(rng.choice([0, 4, 8])) for _ in range(3))
        acc = bool(case % 2)
        label = "case {}: m={} n={} k={} ta={} tb={} count={} pads={} acc={}".format(case, m, n, k, ta, tb, count, pads, acc)
        yield label, (m, n, k, ta, tb, count), pads, acc, group_members(rng, m, n, k, ta, tb, count, pads)


def headroom_sum_items():
    """(label, error of the float32 evaluation against float64, the bound the GPU test applies) for the sum-type bounds
    and the accumulating calls, on the GPU tests' own inputs.  float32 evaluation: NumPy / torch sums and products with
    float32 accumulators, np.add.at into a float32 table."""
    for n in REDUCE_N:
        x = reduce_inputs(n)
        yield ("reduce_sum {}".format(n), abs(float(x.sum(dtype=np.float32)) - x.astype(np.float64).sum()),
               sum_bound(n, float(np.abs(x).max())))
    for b, t, d in TIME_SUM_SHAPES:
        x, dy, base = time_sum_inputs(b, t, d)
        yield ("time_sum {}".format((b, t, d)), float(np.abs(x.sum(1, dtype=np.float32) - x.astype(np.float64).sum(1)).max()),
               sum_bound(t, float(np.abs(x).max())))
    for vocab, e, n, hot in SCATTER_CASES:
        ids, d, base = scatter_inputs(vocab, e, n, hot)
        for skip_pad in (False, True):
            ok = scatter_kept(ids, vocab, skip_pad)
            t32, t64 = base[1:-1].copy(), base[1:-1].astype(np.float64)
            np.add.at(t32, ids[ok], d[ok])
            np.add.at(t64, ids[ok], d[ok].astype(np.float64))
            counts = np.bincount(ids[ok], minlength=vocab)
            bnd = np.array([sum_bound(c + 1, float(np.abs(d).max())) for c in counts])
            yield ("scatter_add V={} n={} skip_pad={}".format(vocab, n, skip_pad), float((np.abs(t32 - t64).max(1) / bnd).max()), 1.0)
    for rows, d in LN_SHAPES:
        r64, r32 = ln_expect(ln_inputs(rows, d), np.float64), ln_expect(ln_inputs(rows, d), np.float32)
        dgamma = np64(r64["dgamma"])
        yield ("layer_norm_bwd {}x{} colsum(dyx)".format(rows, d),
               float(np.abs(r32["dyx"].sum(0).numpy().astype(np.float64) - dgamma).max()), bound(TOL_FUSED, dgamma) * np.sqrt(rows))
    for op in P.EW_OPS:
        for shape in EW_SHAPES:
            a, b, base = ew_inputs(op, shape)
            want = base.astype(np.float64) + ew_expect(op, a, b, np.float64)
            with np.errstate(invalid="ignore"):
                got = base + ew_expect(op, a, b, np.float32)
            yield ("ew {} {} accumulate".format(op, shape), max_err(got, want), bound(TOL_ACT, want))
    for rows, cols in DROPOUT_SHAPES:
        x, base = dropout_inputs(rows, cols)
        want = P.dropout(x, DROPOUT_KEEP, DROPOUT_SALT, 1)
        yield ("dropout {}x{} accumulate".format(rows, cols), max_err(base + want, base.astype(np.float64) + want),
               bound(TOL_ACT, base.astype(np.float64) + want))

    def group(label, k, ta, tb, acc, members):
        worst = 0.0
        for _, _, c0, a, b in members:
            n = b.shape[0] if tb else b.shape[1]
            ref = P.gemm(a.astype(np.float64), b.astype(np.float64), ta, tb) + (c0[:, :n] if acc else 0.0)
            got = P.gemm(a, b, ta, tb) + (c0[:, :n] if acc else np.float32(0.0))
            worst = max(worst, float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6)))
        return label, worst, group_bound(k)
    for m, n, k, ta, tb, count in GROUP_HAND:
        for pads, acc, members in group_hand_runs(m, n, k, ta, tb, count):
            yield group("gemm_group hand {} pads={} acc={}".format((m, n, k, ta, tb, count), pads, acc), k, ta, tb, acc, members)
    for label, (m, n, k, ta, tb, count), pads, acc, members in group_sweep_runs():
        yield group("gemm_group " + label, k, ta, tb, acc, members)
