"""The case table of the truncated sampling step (nm_sample_step): tests/test_sampling_topk_ref.py shows on the CPU
that the float32 restatement meets the rule on it and that the general cases pin the kept set;
tests/test_sampling_topk_kernels_gpu.py holds the kernel to it.

General cases: N(0, 1.5^2) logits, rows 3..37, every vocabulary size at which the kernel changes its path (one column,
fewer columns than a wave, 255 / 256 / 257, unaligned rows of 1001 with ldx = V + 3, more than one round of the
workgroup, the 32000 columns of a translation vocabulary, and LDS_MAX + 1 columns: the first row too long to stay in
LDS), top_k in {0, 1, 2, 40, V, V + 5}, top_p in {1, 0.9, 0.5, 1e-6}, inv_temperature in {1, 1/0.7, 1/2.5}, about a
quarter of the rows finished.  The seeds are chosen so that the band of rule 1 holds ONE admissible kept size in every
row (asserted by the CPU test): the rule pins the kept set, a wrong boundary cannot hide in the band.

C and C_lp.  Measured on the CPU over this table (test_sampling_topk_ref.py): the worst |integer prefix mass - float64
prefix mass| / M of the float32 restatement is E_MASS, its worst logprob error / (1 + |lp|) is E_LP.  The kernel sums
the same integers in any order, so it differs from the restatement only by the last bits of its expf and logf; C and
C_lp are about ten times the measured errors (section 4.9a's C is 13 times its own)."""
from functools import lru_cache
from typing import NamedTuple, Optional

import numpy as np

from . import sampling_ref as SR

LDS_MAX = 36864           # nm_sample_lds_max_columns(): asserted by tests/test_sampling_topk_host.py
E_MASS = 3.874e-8         # measured, see above
E_LP = 9.901e-8
C = 4.0e-7                # 10.3 x E_MASS
C_LP = 1.0e-6             # 10.1 x E_LP
END = 2


class Case(NamedTuple):
    name: str
    rows: int
    v: int
    top_k: int
    top_p: float
    inv_t: float
    seed: int
    pad: int = 0             # ldx = v + pad
    general: bool = True
    salt: int = 0x1234567


IT07, IT25 = 1.0 / 0.7, 1.0 / 2.5

GENERAL = [
    Case("g_v1", 5, 1, 0, 1.0, 1.0, 1),
    Case("g_v1_p05_k2", 3, 1, 2, 0.5, IT07, 2),
    Case("g_v7_k2", 37, 7, 2, 1.0, IT07, 3),
    Case("g_v7_p09", 11, 7, 0, 0.9, 1.0, 4),
    Case("g_v255_k40_p09", 9, 255, 40, 0.9, IT25, 5),
    Case("g_v256_kV_p05", 13, 256, 256, 0.5, 1.0, 6),
    Case("g_v257_kV5_p09", 17, 257, 262, 0.9, IT07, 7),
    Case("g_v257_k1", 6, 257, 1, 1.0, 1.0, 8),
    Case("g_v1001_k40_p05", 23, 1001, 40, 0.5, 1.0, 9, pad=3),
    Case("g_v1001_p1e-6", 7, 1001, 0, 1e-6, IT25, 10, pad=3),
    Case("g_v1001_temp", 8, 1001, 0, 1.0, IT07, 11, pad=3),
    Case("g_v8193_k2_p09", 5, 8193, 2, 0.9, 1.0, 12),
    Case("g_v8193_p05", 4, 8193, 0, 0.5, IT25, 13),
    Case("g_v8193_k40", 6, 8193, 40, 1.0, 1.0, 14),
    Case("g_v32000_p09", 16, 32000, 0, 0.9, 1.0, 315),
    Case("g_v32000_k40_p09", 16, 32000, 40, 0.9, IT07, 16),
    Case("g_v32000_off", 16, 32000, 0, 1.0, 1.0, 17),
    Case("g_vlds1_k40_p09", 4, LDS_MAX + 1, 40, 0.9, 1.0, 18),
    Case("g_vlds1_p05", 4, LDS_MAX + 1, 0, 0.5, IT25, 19),
    Case("g_vlds1_off", 4, LDS_MAX + 1, 0, 1.0, 1.0, 20),
]

TIES = [
    Case("t_uniform_v8_p05", 4, 8, 0, 0.5, 1.0, 31, general=False),
    Case("t_uniform_v300_k5", 5, 300, 5, 1.0, 1.0, 32, general=False),
    Case("t_equal_maxima_k2500", 3, 8193, 2500, 1.0, 1.0, 33, general=False),
    Case("t_equal_maxima_k2500_p05", 3, 8193, 2500, 0.5, IT07, 34, general=False),
    Case("t_unk_columns_p09", 6, 1001, 0, 0.9, 1.0, 35, general=False),
    Case("t_unk_columns_p_almost_1", 6, 1001, 0, 0.9999999, 1.0, 36, general=False),
    Case("t_argmax_alone", 9, 1001, 0, 1e-6, 1.0, 37, general=False),
]

CASES = GENERAL + TIES
BY_NAME = {c.name: c for c in CASES}


class Built(NamedTuple):
    case: Case
    x: np.ndarray            # [rows, v + pad] float32; the logits are x[:, :v]
    finished: np.ndarray     # [rows] int32
    lps: np.ndarray          # [rows] float32
    lens: np.ndarray         # [rows] int32
    ref: SR.RefStep
    exact: Optional[dict]


def _inputs(c: Case):
    rng = np.random.RandomState(c.seed)
    x = np.full((c.rows, c.v + c.pad), np.nan, np.float32)       # the padding must never be read
    x[:, :c.v] = (rng.randn(c.rows, c.v) * 1.5).astype(np.float32)
    fin = (rng.rand(c.rows) < 0.25).astype(np.int32)
    fin[0] = 0
    lps = (-rng.rand(c.rows) * 7).astype(np.float32)
    lens = rng.randint(0, 9, c.rows).astype(np.int32)
    exact = None
    if c.name.startswith("t_uniform"):
        x[:, :c.v] = 0.5
        keep = 4 if c.v == 8 else 5
        allowed = np.zeros((c.rows, c.v), bool)
        allowed[:, :keep] = True
        exact = {"kept": np.full(c.rows, keep), "allowed": allowed}
    elif c.name.startswith("t_equal_maxima"):
        allowed = np.zeros((c.rows, c.v), bool)
        for r in range(c.rows):
            top = np.sort(rng.choice(c.v, 5000, replace=False))
            x[r, :c.v] = np.minimum(x[r, :c.v], 2.0)
            x[r, top] = 3.25
            allowed[r, top[:2500]] = True
        exact = {"allowed": allowed}
        if c.top_p == 1.0:
            exact["kept"] = np.full(c.rows, 2500)
        else:                # 2500 equal terms of 1: the shortest prefix with at least half of their mass
            exact["kept"] = np.full(c.rows, 1250)
    elif c.name.startswith("t_unk_columns"):
        allowed = np.ones((c.rows, c.v), bool)
        for col in (1, 17, 500):
            x[:, col] = -1e9
            allowed[:, col] = False
        exact = {"allowed": allowed}
    elif c.name == "t_argmax_alone":
        allowed = np.zeros((c.rows, c.v), bool)
        allowed[np.arange(c.rows), x[:, :c.v].argmax(1)] = True
        exact = {"kept": np.ones(c.rows, int), "allowed": allowed}
    return x, fin, lps, lens, exact


@lru_cache(maxsize=None)
def build(name: str) -> Built:
    """Inputs and float64 reference of a case: computed once, shared, never written to."""
    c = BY_NAME[name]
    x, fin, lps, lens, exact = _inputs(c)
    ref = SR.ref_step(x[:, :c.v], np.float32(c.inv_t), c.top_k, c.top_p, c.salt, END, fin, lps, lens)
    for a in (x, fin, lps, lens):
        a.setflags(write=False)
    return Built(c, x, fin, lps, lens, ref, exact)
