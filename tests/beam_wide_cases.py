"""The case table of the wide beam step (nm_beam_topk_step_wide, 17 to 64 hypotheses): tests/test_beam_wide_ref.py
establishes on the CPU that the float32 restatement meets the acceptance rule on every case and that the general cases
pin the selected set; tests/test_beam_wide_kernels_gpu.py holds the kernel to it.

The generators, the penalty table and the bound C are those of tests/beam_cases.py (general in k).  Conventions a
case is run in:

  computed   the kernel computes max / lse itself and writes rmax_out / rlse_out
  given      row statistics from ops.row_stats
  tiles64    tile statistics of oracle/beam_ref.py:tile_stats, 64 columns wide
  tiles128   the same, 128 columns wide
  ensemble   log-probabilities with zero row statistics (only the cases built that way)

Measured on the CPU over this table (test_beam_wide_ref.py): worst |float32 restatement - float64| / (1 + |score|)
= 2.62e-7, the lse moved by -2 / 0 / +2 ulp; C = 3.52e-6 is 13 times that.  In every general case, and in its k = 16
twin (same generator and seed), the band at the boundary holds the k-th candidate alone in every sentence.  The largest
first-step |log-probability| of the tie cases is 15.9, below the 30 the rounded-sum rule of exact_selection needs."""
import functools

import numpy as np

from oracle import beam_ref as R

from .beam_cases import C, Case, _general, _tie, penalty_table  # noqa: F401  (C, penalty_table: re-exported)

WIDE = ("computed", "given", "tiles64", "tiles128")


def _cases():
    G = lambda name, roles, k, v, **kw: Case(name, kw.pop("kernels", WIDE), roles, k, v, **kw)
    T = lambda name, tie, k, v, **kw: Case(name, WIDE, "aa", k, v, tie=tie, **kw)
    return [
        G("w_k17_v70", "mfFa", 17, 70, pad=3, seed=101),
        G("w_k32_v516", "mfFae", 32, 516, seed=102),
        G("w_k33_v1000", "mfa", 33, 1000, pad=4, end="last", alpha=0.0, seed=103),
        G("w_k48_v4100", "mfa", 48, 4100, alpha=1.0, seed=104),
        G("w_k64_v2051", "mfFa", 64, 2051, pad=1, seed=105),              # odd V, unaligned rows
        G("w_k64_v32000", "ma", 64, 32000, seed=106),                     # the workload's vocabulary
        G("w_k64_v64", "mfFa", 64, 64, seed=107),
        G("w_k24_v300_ens", "mFa", 24, 300, seed=108, kernels=("ensemble",)),
        G("w_allfin_k40", "FF", 40, 130, seed=109),
        G("w_allend_k20", "ee", 20, 200, seed=110),
        T("t_uniform_same_k17", "uniform_same", 17, 70, seed=120),
        T("t_uniform_apart_k32", "uniform_apart", 32, 64, seed=121),
        T("t_identical_rows_k64", "identical_rows", 64, 129, seed=122),
        T("t_first_step_k64", "first_step", 64, 257, seed=123),
        T("t_ramp_same_k20", "ramp_same", 20, 100, seed=124),
        T("t_ramp_apart_k20", "ramp_apart", 20, 100, seed=125),
        T("t_maxima300_k32", "maxima300", 32, 1000, seed=126),
        T("t_first_step_spill_k64_v40", "first_step", 64, 40, seed=127),  # V < k: 24 picks out of the tie at -1e9
        T("t_uniform_same_k64_v128", "uniform_same", 64, 128, seed=128),  # 8192 equal candidates per sentence
        T("t_identical_rows_k33_v1030", "identical_rows", 33, 1030, pad=2, seed=129),
        T("t_maxima5000_k64", "maxima5000", 64, 6000, seed=130),          # 5000 equal maxima per row
    ]


CASES = _cases()
GENERAL = [c for c in CASES if c.general]
# every general case again at the narrow kernels' widest beam: same generator, same seed
K16 = [Case(c.name + "_at_k16", c.kernels, c.roles, 16, c.v, pad=c.pad, alpha=c.alpha,
            end="last" if c.end == c.v - 1 else c.end, seed=c.seed) for c in GENERAL]
BY_NAME = {c.name: c for c in CASES + K16}
assert len(BY_NAME) == len(CASES) + len(K16)
RUNS = [(c.name, kern) for c in CASES + K16 for kern in c.kernels]


class Built:
    pass


@functools.lru_cache(maxsize=None)
def build(name):
    """Inputs, float64 reference and (tie cases) the exact expectation of a case; computed once per process and left
    unchanged (as tests/beam_cases.py:build, over this table)."""
    c = BY_NAME[name]
    rng = np.random.default_rng(c.seed)
    x, lps, lens, fin = (_general if c.general else _tie)(c, rng)
    o = Built()
    o.case, o.lps, o.lens, o.fin, o.penalty = c, lps, lens, fin, penalty_table(c.alpha)
    if c.ensemble:
        mx, lse = R.row_stats64(x)
        x = ((x.astype(np.float64) - mx[:, None]) - lse[:, None]).astype(np.float32)
        o.rmax = o.rlse = np.zeros(x.shape[0], np.float32)
    else:
        o.rmax = o.rlse = None
    o.logits = x
    o.ref = R.beam_step_ref64(x, c.k, lps, lens, fin, o.penalty, c.end, o.rmax, o.rlse)
    o.exact = None if c.general else R.exact_selection(o.ref)
    for a in (o.logits, o.lps, o.lens, o.fin, o.penalty, o.ref.scores, o.ref.hyp):
        a.setflags(write=False)
    return o
