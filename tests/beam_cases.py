"""The shared case table of the beam step tests: tests/test_beam_ref.py shows on the CPU that a float32 restatement
meets the acceptance rule on every case, tests/test_beam_kernels_gpu.py holds the three kernels to it.

A case fixes the inputs of one step (logits [B*k, V], search state, penalty table, end id), the row stride the
kernels see (``pad`` extra columns of +3e38 behind every row), and the kernels it is run through:

  twopass    ops.row_stats + ops.beam_topk_step
  ensemble   ops.beam_topk_step on log-probabilities with zero row statistics (runners' ensemble path)
  fused      ops.beam_topk_step_fused (falls back to the two-pass kernels for k > 8, V % 4 != 0, unaligned rows,
             V > 131072)
  tiles64    ops.beam_topk_step_tiles on handmade tile statistics, 64 columns wide
  tiles128   the same, 128 columns wide

Sentence roles (one letter per sentence): m = 25% of the hypotheses finished, f = first step (0, -1e9, ...),
F = every hypothesis finished, a = all alive, e = all alive and every pick ends.

``C`` is the bound of the acceptance rule (oracle/beam_ref.py:check_step).  tests/test_beam_ref.py measures the worst
|float32 restatement - float64| / (1 + |score|) over this table, the runs with the float32 lse moved by +-2 ulp
included: 2.13e-7 (MEASURED_F32_ERROR = 2.2e-7 bounds it; the test fails when the table no longer gives a value
within 10% below that).  C = 16 x 2.2e-7 = 3.52e-6,
below the cap 1e-5 that test_kernels_gpu.py::test_beam_topk_step grants, so the cap does not bind.
"""
import functools

import numpy as np

from oracle import beam_ref as R

MEASURED_F32_ERROR = 2.2e-7
C = 16 * MEASURED_F32_ERROR
C_CAP = 1e-5
assert C <= C_CAP
TABLE = 48                                    # penalty table entries: lengths in [0, TABLE - 2]
ALL = ("twopass", "fused", "tiles64", "tiles128")


class Case:
    def __init__(self, name, kernels, roles, k, v, pad=0, alpha=0.6, end=2, seed=0, tie=None, scale=4.0):
        self.name, self.kernels, self.roles, self.k, self.v, self.pad = name, tuple(kernels), roles, k, v, pad
        self.alpha, self.seed, self.tie, self.scale = alpha, seed, tie, scale
        self.end = v - 1 if end == "last" else end
        self.b = len(roles)
        self.ensemble = self.kernels == ("ensemble",)

    general = property(lambda self: self.tie is None)


def penalty_table(alpha):
    """ops.length_penalty_table's float32 values."""
    lens = np.arange(TABLE, dtype=np.float32)
    return (((np.float32(5.0) + lens) / np.float32(6.0)) ** np.float32(alpha)).astype(np.float32)


def _state(rng, roles, k):
    b = len(roles)
    lps = (-rng.random((b, k)) * 30).astype(np.float32)
    lens = rng.integers(0, TABLE - 1, size=(b, k)).astype(np.int32)
    fin = np.zeros((b, k), bool)
    for s, role in enumerate(roles):
        if role == "m":
            fin[s] = rng.random(k) < 0.25
            if k > 1:                          # at least one finished and one live hypothesis
                one, other = rng.choice(k, size=2, replace=False)
                fin[s, one], fin[s, other] = True, False
        elif role == "F":
            fin[s] = True
        elif role == "f":
            lps[s, 0], lps[s, 1:], lens[s] = 0.0, -1e9, 0
        elif role == "e":
            lps[s], lens[s] = (-rng.random(k) * 5).astype(np.float32), lens[s, 0]
    return lps, lens, fin


def _general(c, rng):
    rows = c.b * c.k
    x = (rng.standard_normal((rows, c.v)) * c.scale).astype(np.float32)
    lps, lens, fin = _state(rng, c.roles, c.k)
    for r in range(rows):                      # a logit planted at end_id: new finished flags arise
        role = c.roles[r // c.k]
        if role == "e":
            x[r, c.end] = x[r].max() + np.float32(40.0)
        elif role in "ma" and r % 3 == 0:
            x[r, c.end] = x[r].max() + np.float32(2.0)
    return x, lps, lens, fin


def _spread_state(rng, b, k, same):
    """Live rows whose beams are identical (``same``) or lie far apart: sums 1.5 apart, best beam in the middle."""
    lens = np.tile(rng.integers(0, 8, size=(b, 1)), (1, k)).astype(np.int32)
    if same:
        lps = np.tile((-rng.random((b, 1)) * 20).astype(np.float32), (1, k))
    else:
        order = np.roll(np.arange(k), k // 2)
        lps = (-1.5 * order[None, :] - rng.integers(0, 8, size=(b, 1))).astype(np.float32)
    return lps, lens, np.zeros((b, k), bool)


def _tie(c, rng):
    rows, k, v, kind = c.b * c.k, c.k, c.v, c.tie
    if kind in ("uniform_same", "uniform_apart"):
        x = np.zeros((rows, v), np.float32)
        return (x,) + _spread_state(rng, c.b, k, kind == "uniform_same")
    if kind == "identical_rows":
        one = (rng.standard_normal((c.b, 1, v)) * 2).astype(np.float32)
        return (np.tile(one, (1, k, 1)).reshape(rows, v),) + _spread_state(rng, c.b, k, True)
    if kind == "first_step":
        x = (rng.standard_normal((rows, v)) * 2).astype(np.float32)
        lps = np.tile(np.array([0.0] + [-1e9] * (k - 1), np.float32), (c.b, 1))
        return x, lps, np.zeros((c.b, k), np.int32), np.zeros((c.b, k), bool)
    if kind in ("ramp_same", "ramp_apart"):
        x = np.tile(np.float32(1e-3) * np.arange(v, dtype=np.float32), (rows, 1))
        return (x,) + _spread_state(rng, c.b, k, kind == "ramp_same")
    x = rng.standard_normal((rows, v)).astype(np.float32)
    if kind.startswith("maxima"):              # maxima256 / maxima257: the candidate list exactly full / overflowing
        n = int(kind[6:])
        for r in range(rows):
            x[r, rng.choice(v, size=n, replace=False)] = 30.0
    else:                                      # tilesN_W: one equal maximum in each of N tiles of width W
        n, w = (int(t) for t in kind[5:].split("_"))
        assert v == 65 * w
        for r in range(rows):
            tiles = rng.choice(65, size=n, replace=False)
            x[r, tiles * w + rng.integers(0, w, size=n)] = 30.0
    return (x,) + _spread_state(rng, c.b, k, False)


class Built:
    pass


@functools.lru_cache(maxsize=None)
def build(name):
    """Inputs, float64 reference and (tie cases) the exact expectation of a case; computed once per process."""
    c = BY_NAME[name]
    rng = np.random.default_rng(c.seed)
    x, lps, lens, fin = (_general if c.general else _tie)(c, rng)
    o = Built()
    o.case, o.lps, o.lens, o.fin, o.penalty = c, lps, lens, fin, penalty_table(c.alpha)
    if c.ensemble:                             # the averaged log-probabilities the ensemble runner hands over
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


def _cases():
    G = Case
    out = [
        # V < k: the lists hold padding entries (no first-step sentence: its spill is a structural tie, below)
        G("v4_k5", ALL, "mFa", 5, 4, seed=1), G("v4_k8", ALL, "maF", 8, 4, pad=4, alpha=1.0, end="last", seed=2),
        G("v4_k5_ens", ("ensemble",), "mFa", 5, 4, seed=3),
        # no V % 4 requirement in the two-pass and tile kernels; the fused entry point falls back
        G("v17_k1", ALL, "mfFa", 1, 17, seed=4, alpha=0.0), G("v17_k2", ALL, "mfF", 2, 17, pad=3, seed=5, end="last"),
        G("v129_k9", ALL, "mfF", 9, 129, seed=6), G("v129_k16", ALL, "mfa", 16, 129, pad=3, alpha=1.0, seed=7),
        G("v129_k4_ens", ("ensemble",), "mfF", 4, 129, pad=4, alpha=0.0, seed=8),
        # last partial tile at both widths, fewer tiles than K
        G("v64_k4", ALL, "mfF", 4, 64, seed=9), G("v68_k5", ALL, "mfa", 5, 68, pad=4, end="last", seed=10),
        G("v128_k8", ALL, "mfF", 8, 128, alpha=0.0, seed=11), G("v132_k9", ALL, "mfa", 9, 132, end="last", seed=12),
        G("v260_k16", ALL, "mfF", 16, 260, pad=4, alpha=1.0, end="last", seed=13),
        G("v260_k2", ALL, "mfa", 2, 260, pad=3, end="last", seed=14),
        G("v516_k16", ALL, "mfFa", 16, 516, seed=15), G("v516_k1", ALL, "mfFa", 1, 516, pad=4, end="last", seed=16),
        G("v1000_k5", ALL, "mfF", 5, 1000, pad=4, end="last", alpha=0.0, seed=17),
        G("v1000_k9", ALL, "mfa", 9, 1000, pad=3, seed=18), G("v1000_k8_ens", ("ensemble",), "mfa", 8, 1000, seed=19),
        # one or two slices per row in the two-pass kernel
        G("v4096_k4", ALL, "mfF", 4, 4096, seed=20), G("v4100_k8", ALL, "mfa", 8, 4100, pad=4, end="last", seed=21),
        G("v4100_k16", ("twopass", "fused"), "mfF", 16, 4100, pad=3, alpha=1.0, seed=22),
        # every pick ends (all_finished stays 1); every input finished (the step sorts the state and emits <pad>)
        G("every_pick_ends", ALL, "e", 4, 260, end="last", seed=23), G("every_pick_ends_k9", ALL, "e", 9, 68, seed=24),
        G("all_inputs_finished", ALL, "FFF", 5, 132, alpha=1.0, seed=25),
        G("all_inputs_finished_80_rows", ALL, "F" * 10, 8, 64, seed=26),
        G("all_inputs_finished_ens", ("ensemble",), "FF", 9, 17, seed=27),
        # row_scan_nv 8 -> 16 -> 32 -> fallback; 1024 -> 1025 tiles at width 64 and at width 128
        G("v32768_k8", ("fused", "tiles128"), "mf", 8, 32768, seed=28),
        G("v32772_k4", ("fused", "twopass"), "mf", 4, 32772, pad=4, end="last", seed=29),
        G("v65536_k4", ("fused", "tiles64", "tiles128"), "mf", 4, 65536, end="last", seed=30),
        G("v65540_k5", ("fused", "tiles64", "tiles128"), "ma", 5, 65540, pad=4, end="last", seed=31),
        G("v131072_k4", ("fused", "tiles64", "tiles128"), "mf", 4, 131072, end="last", alpha=1.0, seed=32),
        G("v131076_k5", ("fused", "tiles64", "tiles128", "twopass"), "mf", 5, 131076, end="last", seed=33),
    ]
    T = lambda name, kernels, b, k, v, tie, **kw: Case(name, kernels, "a" * b, k, v, tie=tie, **kw)
    out += [
        T("tie_uniform_same_k5", ALL, 2, 5, 260, "uniform_same", seed=40),
        T("tie_uniform_apart_k9", ALL, 2, 9, 132, "uniform_apart", seed=41, pad=4),
        T("tie_uniform_same_k1", ALL, 2, 1, 17, "uniform_same", seed=42),
        T("tie_identical_rows_k4", ALL, 3, 4, 1000, "identical_rows", seed=43),
        T("tie_identical_rows_k16", ALL, 2, 16, 516, "identical_rows", seed=44, pad=3),
        T("tie_identical_rows_ens", ("ensemble",), 2, 8, 129, "identical_rows", seed=45),
        T("tie_first_step_v4_k5", ALL, 2, 5, 4, "first_step", seed=46),
        T("tie_first_step_v4_k8", ALL, 2, 8, 4, "first_step", seed=47, alpha=1.0),
        T("tie_first_step_v4_k16", ALL, 2, 16, 4, "first_step", seed=48, pad=4),
        T("tie_maxima256_k5", ALL, 2, 5, 4096, "maxima256", seed=49),
        T("tie_maxima257_k5", ALL, 2, 5, 4096, "maxima257", seed=50),
        T("tie_maxima256_k16", ("twopass", "tiles64", "tiles128"), 1, 16, 1000, "maxima256", seed=51),
        T("tie_maxima257_k8", ALL, 1, 8, 1000, "maxima257", seed=52, pad=4),
        T("tie_tiles64_w64", ("tiles64", "fused"), 2, 4, 65 * 64, "tiles64_64", seed=53),
        T("tie_tiles65_w64", ("tiles64", "twopass"), 2, 4, 65 * 64, "tiles65_64", seed=54),
        T("tie_tiles64_w128", ("tiles128", "fused"), 2, 8, 65 * 128, "tiles64_128", seed=55),
        T("tie_tiles65_w128", ("tiles128", "twopass"), 2, 9, 65 * 128, "tiles65_128", seed=56),
        T("tie_ramp_apart_k4", ALL, 2, 4, 4096, "ramp_apart", seed=57),
        T("tie_ramp_same_k8", ALL, 1, 8, 1000, "ramp_same", seed=58),
        T("tie_ramp_apart_k16", ("twopass", "tiles64", "tiles128"), 1, 16, 1000, "ramp_apart", seed=59, pad=3),
    ]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RUNS = [(c.name, kern) for c in CASES for kern in c.kernels]

# the one case that goes through the real nm_logits_stats_gemm: more than 256 rows, so the library itself picks
# 128-column tiles
GEMM_CASE = Case("gemm_v260_k8_33_sentences", ("tiles_gemm",), "mfFa" * 8 + "m", 8, 260, end="last", seed=60)
BY_NAME[GEMM_CASE.name] = GEMM_CASE
