"""Case table and float64 reference of the decoder-step GEMM groups (nm_step_group, csrc/nm_step.hip), shared by the
GPU sweep (tests/test_step_group_sweep_gpu.py: every kernel instance against float64) and the CPU check of the table
itself (tests/test_step_group_cases.py: the instance each case was written for is the one the library's own rule --
nm_step_group_plan -- names, every instance is reached, every dispatch boundary from both sides).

A case is (name, M, problems, instance under NM_STEP_DMA=0, instance under NM_STEP_DMA=1); a problem is
(N, K, epilogue, act, bias?, add?, ids?, in place?).  Instances are named as ops.STEP_GROUP_PLANS names them.

What the shapes are for (the slices are those of the kernels: 16 waves x trips of 64 k (one row tile) or 32 k (two), and
4 or 8 waves x trips of 32 k on the 32x32 tiles):
  K = 48    three 16-k slices, thirteen idle waves; on 32x32 tiles one and a half trips for wave 0 alone
  K = 272   17 x 16: 16-row kernels 32 k per wave, the last waves idle; 32x32 tiles: 8.5 trips, the half trip ends a slice
  K = 1104  69 x 16: 80 k per wave (a trip of 64 + 16), wave 13 ends inside a trip, waves 14 and 15 idle;
            32x32 tiles with 8 waves: 160 k per wave, wave 6 has 4.5 trips, wave 7 none
  K = 16    less than one trip everywhere
  K = 112   32x32 tiles with 4 waves: 32 k per wave, ALL four waves busy, the last one on half a trip
  K = 240   32x32 tiles with 8 waves: the same with all eight
  K = 496   31 x 16: 16-row kernels 32 k per wave, ALL sixteen waves busy, the last one on 16 k;
            32x32 tiles: 128 k (4 waves) or 64 k (8 waves) per wave, the last wave ends on a half trip
(With 48, 272 and 1104 alone the LAST slice of every kernel would be empty in every case: a reduction that dropped it
would pass.)
Inputs are scaled as test_gemm (tests/test_kernels_gpu.py) scales them: A by 1 / sqrt(K), so sums are O(1)."""
import collections
import functools
import zlib

import numpy as np

Prob = collections.namedtuple("Prob", "n k epilogue act bias add ids inplace")
Case = collections.namedtuple("Case", "name m probs want want_dma")

PLAIN, GATES, CAND = 0, 1, 2
TABLE_ROWS = 11            # rows of an `add` / `xc` table that row ids index
PAD_ROWS, PAD_COLS = 8, 4  # NaN-filled rows below / columns beside every output
IN_W = 8                   # width of the input half of an in-place state row [input | state | pad]

# the project's own bounds (test_gemm: the same exact-fp32 MFMA sums), of the largest reference magnitude
TOL_ACT = 1e-5             # tanh, gate and blend epilogues


def tol_plain(k):
    return 2e-6 * np.sqrt(k) + 1e-6


def P(n, k, epilogue=PLAIN, act=0, bias=True, add=False, ids=False, inplace=False):
    return Prob(n, k, epilogue, act, bias or epilogue == GATES, add, ids, inplace)


def C(name, m, probs, want, want_dma=None):
    return Case(name, m, tuple(probs), want, want_dma or want)


CASES = (
    # ---- step_group_medium_kernel<4,2,2>: M > 256, at least 256 tiles of 64x64 -------------------------------------
    # 260 rows = 4 full row tiles + 4 rows: the second 32-row sub-tile of the last workgroup row is EMPTY; 1552 = 24 x 64
    # + 16, 1040 = 16 x 64 + 16, 656 = 10 x 64 + 16: the second 32-column sub-tile of each last workgroup column too.
    # 5 x (25 + 17 + 11) = 265 tiles.  Gates (with a row-indexed table) + two plain products, as group 1 of a beam step
    C("fat-gates-ids-3", 260, [P(1552, 48, GATES, add=True, ids=True), P(1040, 16), P(656, 272, bias=False)],
      "medium-4x2x2"),
    # one row past the boundary (sub-tile rows 1 of 32, then empty), N = 51 x 64 + 36: candidate + blend IN PLACE with a
    # row-indexed xc table and the history copy, as group 2 of a beam step.  5 x 52 = 260 tiles
    C("fat-cand-inplace-257", 257, [P(3300, 48, CAND, ids=True, inplace=True)], "medium-4x2x2"),
    C("fat-plain-300", 300, [P(3300, 48, act=1, add=True)], "medium-4x2x2"),          # 300 = 4 x 64 + 44: both sub-tiles partial
    # exactly 256 tiles (8 x 32), N = 2040 is no multiple of 4 (rows of C and add at odd alignments); partner: 248 tiles
    C("fat-256-tiles", 512, [P(2040, 16)], "medium-4x2x2"),
    C("thin-248-tiles", 512, [P(1984, 16)], "medium-4x1x1"),
    C("thin-255-tiles", 257, [P(3264, 16, bias=False)], "medium-4x1x1"),               # 5 x 51 = 255 tiles of 64x64
    C("fat-all-slices", 260, [P(3300, 112)], "medium-4x2x2"),
    # ---- step_group_medium_kernel<8,1,1> / <4,1,1>: grid of 32x32 tiles <= 640 / > 640 ----------------------------
    C("grid-640", 320, [P(2048, 48)], "medium-8x1x1"),                                 # 10 x 64
    C("grid-650", 320, [P(2080, 48, act=1, add=True, ids=True)], "medium-4x1x1"),      # 10 x 65
    C("grid-640-ragged", 289, [P(2048, 48, act=1)], "medium-8x1x1"),                   # 289 = 9 x 32 + 1
    C("k8-1104", 257, [P(40, 1104)], "medium-8x1x1"),
    C("k8-cand-272-16", 257, [P(36, 272, CAND, ids=True), P(20, 16, add=True, ids=True)], "medium-8x1x1"),
    C("k8-all-slices", 257, [P(40, 240), P(36, 496, act=1)], "medium-8x1x1"),
    C("thin-all-slices", 320, [P(2080, 112)], "medium-4x1x1"),
    # ---- step_group_kernel<16,1,0> / <16,2,0>: M <= 256, at most / more than 512 tiles of 16x16 ----------------------
    C("tiles-512", 256, [P(512, 16)], "16x1"),                                         # 16 x 32
    C("tiles-513", 137, [P(912, 16, act=1)], "16x2"),                                  # 9 x 57; 137 = 4 x 32 + 9
    C("tiles-528", 256, [P(528, 16)], "16x2"),                                         # 16 x 33
    # 100 = 3 x 32 + 4: the second row tile of the last workgroup row is EMPTY, the first partial
    C("two-tiles-1104", 100, [P(1184, 1104)], "16x2"),
    C("two-tiles-48", 100, [P(1200, 48, GATES, add=True)], "16x2"),
    # 250 = 7 x 32 + 26: the second row tile is partial (10 of 16 rows)
    C("two-tiles-gates-ids", 250, [P(36, 1104, GATES, add=True, ids=True), P(500, 272, act=1)], "16x2"),
    C("one-tile-tiny", 19, [P(20, 16, GATES)], "16x1"),
    C("one-tile-cand-ids", 37, [P(40, 272, CAND, ids=True, inplace=True), P(24, 1104, add=True, ids=True)], "16x1"),
    C("one-tile-all-slices", 37, [P(40, 496), P(24, 256, act=1)], "16x1"),
    C("two-tiles-all-slices", 100, [P(1200, 496)], "16x2"),
    # ---- step_group_dma_kernel (NM_STEP_DMA=1, every K a multiple of 64): three chunks in flight over four images -----
    # 5, 1 and 3 chunks: the prologue deeper than the loop, and the first wrap of the ring (chunk 4 into image 0)
    C("dma-5-1-3", 257, [P(704, 320, add=True, ids=True), P(36, 64, act=1), P(100, 192)], "medium-8x1x1", "dma"),
    # 2 and 4 chunks; gates and candidate epilogues of the DMA kernel
    C("dma-2-4", 330, [P(70, 128, GATES, add=True, ids=True), P(40, 256, CAND, ids=True, inplace=True)],
      "medium-8x1x1", "dma"),
    # one K of the group is no multiple of 64: the whole group falls back to the register-staged kernel
    C("dma-refused-k-48", 330, [P(70, 128), P(40, 48)], "medium-8x1x1", "medium-8x1x1"),
)

# a planted permutation per a_kind-0 instance: (name, M, N, K, instance, needs NM_STEP_DMA=1).  K = 496 keeps every K
# slice of every kernel busy (above); the DMA kernel does not split K: five chunks
PERMUTATIONS = (
    ("perm-fat", 260, 3300, 496, "medium-4x2x2", False),
    ("perm-8", 260, 40, 496, "medium-8x1x1", False),
    ("perm-4", 260, 2300, 496, "medium-4x1x1", False),          # 9 x 72 = 648 tiles of 32x32, 5 x 36 of 64x64
    ("perm-16x1", 100, 40, 496, "16x1", False),
    ("perm-16x2", 100, 1200, 496, "16x2", False),
    ("perm-dma", 260, 100, 320, "dma", True),
)
PERM_STRIDE = 37           # row i has its single 1 in column 37 i mod K (37 divides no K above: all columns distinct)

# a_kind 1 (the split-S attention partials merged in the operand loader): (key batches, queries per key batch, source
# length, attention width, context width = K, N).  12 source positions per partial: 70 -> 6, 96 -> 8 partials (the
# 8-wide loader); 97 -> 9, refused
PARTIALS = ((19, 1, 70, 32, 48, 20), (7, 3, 70, 32, 48, 20), (19, 1, 96, 32, 48, 20), (7, 3, 96, 32, 272, 36))
PARTIALS_REFUSED = (5, 1, 97, 32, 48, 20)


def cdiv(a, b):
    return -(-a // b)


def tile_counts(case):
    """Shape arithmetic only -- (16x16 tiles, 64x64 tiles, 32x32 tiles) of the group; WHICH kernel these numbers select
    is asked of the library (nm_step_group_plan), never restated here."""
    return tuple(sum(cdiv(case.m, t) * cdiv(p.n, t) for p in case.probs) for t in (16, 64, 32))


def normal(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def row_ids(rng, m):
    """Ids into an 11-row table: they repeat (m > 11), and the first and the last row of the problem -- different
    workgroup tiles whenever there is more than one -- share id 3."""
    ids = rng.integers(0, TABLE_ROWS, m).astype(np.int32)
    ids[0] = ids[m - 1] = 3
    return ids


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def reference(m, p, x):
    """float64 results of one problem from its float32 inputs: {output name: [m, n'] array}.
    plain: act(A . Bt^T + bias + add[ids]); gates: sigmoid(.) and r*h; candidate: tanh(xc[ids] + .), u*h + (1-u)*c."""
    f = lambda a: np.asarray(a, np.float64)
    s = f(x["A"][:, :p.k]) @ f(x["Bt"][:, :p.k]).T
    rows = x["ids"] if p.ids else np.arange(m)
    if p.epilogue == CAND:
        c = np.tanh(f(x["xc"])[rows, :p.n] + s)
        u = f(x["ru_in"])[:, p.n:]
        hn = u * f(x["h"]) + (1.0 - u) * c
        return {"h_out": hn, "h_out2": hn}
    if p.bias:
        s = s + f(x["bias"])
    if p.add:
        s = s + f(x["add"])[rows, :p.n]
    if p.epilogue == GATES:
        gate = sigmoid(s)
        return {"ru": gate, "rh": gate[:, :p.n // 2] * f(x["h"])}
    return {"C": np.tanh(s) if p.act else s}


@functools.lru_cache(maxsize=None)
def problem_data(name, m, index, p):
    """(inputs, float64 reference, bound) of problem `index` of a case; built once per process and never modified
    (the tests upload copies)."""
    rng = np.random.default_rng([zlib.crc32(name.encode()), index])
    x = {"A": normal(rng, (m, p.k + 8), 1.0 / np.sqrt(p.k)),             # lda > K
         "Bt": normal(rng, (p.n, p.k + 4 * (index % 2)))}                # ldb > K on every other problem
    if p.bias:
        x["bias"] = normal(rng, p.n)
    if p.ids:
        x["ids"] = row_ids(rng, m)
    table_rows = TABLE_ROWS if p.ids else m
    if p.add:
        x["add"] = normal(rng, (table_rows, p.n + PAD_COLS))
    if p.epilogue == GATES:
        x["h"] = normal(rng, (m, p.n // 2))
    if p.epilogue == CAND:
        x["xc"] = normal(rng, (table_rows, p.n + PAD_COLS))
        x["ru_in"] = rng.uniform(0.02, 0.98, (m, 2 * p.n)).astype(np.float32)
        x["h"] = normal(rng, (m, p.n))
        x["input_half"] = normal(rng, (m, IN_W))
    for a in x.values():
        a.setflags(write=False)
    ref = reference(m, p, x)
    tol = tol_plain(p.k) if (p.epilogue == PLAIN and not p.act) else TOL_ACT
    return x, ref, tol


def case_data(case):
    return [problem_data(case.name, case.m, i, p) for i, p in enumerate(case.probs)]


def placeholder_specs(case):
    """Descriptors of a case with made-up (aligned, never dereferenced) addresses: what nm_step_group_plan needs to
    name the kernel -- shapes, leading dimensions and which optional operands are present."""
    addr = 0x10000
    specs = []
    for i, p in enumerate(case.probs):
        s = dict(A=addr, lda=p.k + 8, Bt=addr, ldb=p.k + 4 * (i % 2), N=p.n, K=p.k, epilogue=p.epilogue, act=p.act)
        if p.bias and p.epilogue != CAND:
            s["bias"] = addr
        if p.add and p.epilogue != CAND:
            s.update(add=addr, ldadd=p.n + PAD_COLS)
            if p.ids:
                s["add_ids"] = addr
        if p.epilogue == PLAIN:
            s.update(C=addr, ldc=p.n + PAD_COLS)
        elif p.epilogue == GATES:
            s.update(h=addr, ldh=p.n // 2, ru=addr, rh=addr)
        else:
            s.update(xc=addr, ldxc=p.n + PAD_COLS, ru=addr, h=addr, ldh=IN_W + p.n + PAD_COLS, h_out=addr,
                     ldho=IN_W + p.n + PAD_COLS, h_out2=addr, ldho2=p.n + PAD_COLS)
            if p.ids:
                s["xc_ids"] = addr
        specs.append(s)
    return specs


def partials_reference(pctx, pstat, energies, mask_rows):
    """What the a_kind-1 loader and the weight-writing workgroups compute from the split-S workspace, in float64
    (attention/feed_forward.py:139-154 carried through the partial statistics {max, sum exp, sum exp * mask, -}):
    f_i = exp(m_i - M), den = sum f_i lm_i + 1e-8 sum f_i la_i; context = sum f_i pctx_i / den, weights = exp(e - M)
    mask / den."""
    pctx, pstat, energies = (np.asarray(a, np.float64) for a in (pctx, pstat, energies))
    big = pstat[:, :, 0].max(1, keepdims=True)
    f = np.exp(pstat[:, :, 0] - big)
    den = (f * pstat[:, :, 2]).sum(1) + 1e-8 * (f * pstat[:, :, 1]).sum(1)
    ctx = (f[:, :, None] * pctx).sum(1) / den[:, None]
    weights = np.exp(energies - big) * np.asarray(mask_rows, np.float64) / den[:, None]
    return ctx, weights
