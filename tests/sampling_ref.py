"""The rule of the truncated sampling step (nm_sample_step, include/nmhip_sample.h) restated twice:

``ref_step``   z = x * inv_temperature is the float32 product, everything after it float64: the order (z descending,
               column ascending), the cumulative softmax masses along it, the top-k prefix and its mass M, the nucleus
               boundary, the restated Gumbel noise (oracle/nm_oracle.py:gumbel_noise);
``f32_step``   the kernel's arithmetic: float32 exp, the fixed-point terms round(exp(z - max) * 2^31) summed in
               integers, target = ceil(top_p * M) in float64, float32 logarithms;
``check_step`` accepts an engine result against ``ref_step`` (the four conditions below).

The oracle package is frozen, so the restatement lives with the tests."""
import math
from typing import List, NamedTuple, Optional

import numpy as np

from oracle.nm_oracle import gumbel_noise

SCALE = 2.0 ** 31
DRAW_GAP = 1e-4       # tests/test_sampling_gpu.py: float32 logs differ in the last bit between two implementations


class RefStep(NamedTuple):
    z: np.ndarray            # [rows, V] float32
    order: np.ndarray        # [rows, V] columns by (z descending, column ascending)
    cum: np.ndarray          # [rows, V] float64 masses of the prefixes, exp(z - max) units
    kk: int                  # size of the top-k prefix
    mass: np.ndarray         # [rows] float64 M, the mass of the top-k prefix
    top_p: float             # the float32 value
    kept: np.ndarray         # [rows] the rule's kept size
    noise: np.ndarray        # [rows, V] float32
    zmax: np.ndarray         # [rows] float64
    end: int
    finished: np.ndarray
    logprob_sum: np.ndarray
    lengths: np.ndarray


class StepOut(NamedTuple):
    symbol: np.ndarray
    logprob: np.ndarray
    kept: np.ndarray
    finished: np.ndarray
    logprob_sum: np.ndarray
    lengths: np.ndarray


def scaled(x: np.ndarray, inv_temperature) -> np.ndarray:
    return (x.astype(np.float32) * np.float32(inv_temperature)).astype(np.float32)


def ordered(z: np.ndarray) -> np.ndarray:
    return np.argsort(-z.astype(np.float64), axis=1, kind="stable")


def prefix_size(top_k: int, vocab: int) -> int:
    return top_k if 1 <= top_k < vocab else vocab


def ref_step(x, inv_temperature, top_k, top_p, salt, end, finished, logprob_sum, lengths) -> RefStep:
    z = scaled(x, inv_temperature)
    rows, vocab = z.shape
    order = ordered(z)
    zs = np.take_along_axis(z, order, 1).astype(np.float64)
    cum = np.cumsum(np.exp(zs - zs[:, :1]), axis=1)
    kk = prefix_size(top_k, vocab)
    mass = cum[:, kk - 1].copy()
    p = float(np.float32(top_p))
    if p == 1.0:
        kept = np.full(rows, kk)
    else:
        kept = np.array([int(np.searchsorted(cum[r, :kk], p * mass[r], side="left")) + 1 for r in range(rows)])
        kept = np.minimum(kept, kk)
    return RefStep(z, order, cum, kk, mass, p, kept, gumbel_noise(rows, vocab, salt), zs[:, 0], end,
                   np.asarray(finished), np.asarray(logprob_sum, np.float32), np.asarray(lengths))


def admissible(ref: RefStep, r: int, c: float) -> List[int]:
    """Every kept size the band of rule 1 admits in row r."""
    if ref.top_p == 1.0:
        return [ref.kk]
    cum, m = ref.cum[r, :ref.kk], ref.mass[r]
    before = np.concatenate([[0.0], cum[:-1]])
    ok = (before < ref.top_p * m + c * m) & (cum >= ref.top_p * m - c * m)
    return (np.nonzero(ok)[0] + 1).tolist()


def _draw(ref_z, noise, prefix):
    noisy = (ref_z[prefix] + noise[prefix]).astype(np.float32)
    best = noisy.max()
    return noisy, best, int(prefix[noisy == best].min())


def check_step(ref: RefStep, got: StepOut, c: float, c_lp: float, exact: Optional[dict] = None):
    """(errors, exact draws, live rows).  An engine result is accepted when, in every unfinished row,
    1. kept is admissible: the float64 mass of the first kept - 1 entries is < top_p*M + C*M, that of the first kept
       entries >= top_p*M - C*M, and kept <= top_k when top-k is on (with the nucleus off: kept is the prefix size);
    2. the symbol lies in that prefix and maximises z + noise (float32) over it up to DRAW_GAP;
    3. logprob is within C_lp * (1 + |lp|) of the float64 value over the engine's own prefix;
    4. the state outputs are exact; a finished row emits <pad>, 0, 0 and copies its state."""
    errors, hits, live = [], 0, 0
    rows = ref.z.shape[0]
    for r in range(rows):
        if ref.finished[r]:
            if (got.symbol[r], got.logprob[r], got.kept[r]) != (0, 0.0, 0):
                errors.append("row {}: finished row emitted {}".format(r, (got.symbol[r], got.logprob[r], got.kept[r])))
            if (got.finished[r], got.lengths[r]) != (1, ref.lengths[r]) or got.logprob_sum[r] != ref.logprob_sum[r]:
                errors.append("row {}: finished row's state moved".format(r))
            continue
        live += 1
        k, sym = int(got.kept[r]), int(got.symbol[r])
        if k not in admissible(ref, r, c):
            errors.append("row {}: kept {} not admissible {} (rule {})".format(r, k, admissible(ref, r, c), ref.kept[r]))
            continue
        if exact is not None and "kept" in exact and k != exact["kept"][r]:
            errors.append("row {}: kept {} != exact {}".format(r, k, exact["kept"][r]))
        prefix = ref.order[r, :k]
        if sym not in prefix:
            errors.append("row {}: symbol {} outside the kept prefix of {}".format(r, sym, k))
            continue
        if exact is not None and "allowed" in exact and not exact["allowed"][r, sym]:
            errors.append("row {}: symbol {} not allowed".format(r, sym))
        noisy, best, want = _draw(ref.z[r], ref.noise[r], prefix)
        mine = float(noisy[np.nonzero(prefix == sym)[0][0]])
        if not best - mine <= DRAW_GAP:
            errors.append("row {}: symbol {} falls short of the maximum by {}".format(r, sym, best - mine))
        hits += int(sym == want)
        lp = (float(ref.z[r, sym]) - ref.zmax[r]) - math.log(ref.cum[r, k - 1])
        if not abs(float(got.logprob[r]) - lp) <= c_lp * (1.0 + abs(lp)):
            errors.append("row {}: logprob {} vs {}".format(r, got.logprob[r], lp))
        if got.finished[r] != int(sym == ref.end) or got.lengths[r] != ref.lengths[r] + 1:
            errors.append("row {}: finished / lengths".format(r))
        if got.logprob_sum[r] != np.float32(ref.logprob_sum[r]) + np.float32(got.logprob[r]):
            errors.append("row {}: logprob_sum".format(r))
    return errors, hits, live


def f32_terms(z: np.ndarray) -> np.ndarray:
    """round(exp(z - max) * 2^31) with the float32 exponential, as integers; [rows, V] in column order."""
    mx = z.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.where(z == mx, np.float32(1.0), np.exp((z - mx).astype(np.float32)).astype(np.float32))
    return np.rint(e.astype(np.float64) * SCALE).astype(np.int64)


def f32_masses(x, inv_temperature):
    """(order, integer prefix masses along it) of the kernel's arithmetic."""
    z = scaled(x, inv_temperature)
    order = ordered(z)
    return z, order, np.cumsum(np.take_along_axis(f32_terms(z), order, 1), axis=1)


def f32_step(x, inv_temperature, top_k, top_p, salt, end, finished, logprob_sum, lengths) -> StepOut:
    z, order, cum = f32_masses(x, inv_temperature)
    rows, vocab = z.shape
    kk = prefix_size(top_k, vocab)
    p = float(np.float32(top_p))
    noise = gumbel_noise(rows, vocab, salt)
    finished, lengths = np.asarray(finished), np.asarray(lengths)
    lps = np.asarray(logprob_sum, np.float32)
    out = StepOut(np.zeros(rows, np.int32), np.zeros(rows, np.float32), np.zeros(rows, np.int32),
                  np.ones(rows, np.int32), lps.copy(), lengths.astype(np.int32).copy())
    for r in range(rows):
        if finished[r]:
            continue
        kept = kk
        if p < 1.0:
            m = int(cum[r, kk - 1])
            target = min(max(int(math.ceil(p * float(m))), 1), m)
            kept = int(np.searchsorted(cum[r, :kk], target, side="left")) + 1
        prefix = order[r, :kept]
        _, _, sym = _draw(z[r], noise[r], prefix)
        total = np.float32(float(int(cum[r, kept - 1])) * (1.0 / SCALE))
        lp = np.float32(np.float32(z[r, sym] - z[r].max()) - np.log(total, dtype=np.float32))
        out.symbol[r], out.logprob[r], out.kept[r] = sym, lp, kept
        out.finished[r] = int(sym == end)
        out.lengths[r] = lengths[r] + 1
        out.logprob_sum[r] = lps[r] + lp
    return out


def f32_errors(x, inv_temperature, top_k, top_p, finished):
    """(worst |integer prefix mass - float64 prefix mass| / M over the top-k prefix, worst logprob error / (1 + |lp|)
    over every entry of the rule's kept prefix) of the float32 restatement on the unfinished rows."""
    z, order, cum_i = f32_masses(x, inv_temperature)
    ref = ref_step(x, inv_temperature, top_k, top_p, 0, -1, finished, np.zeros(len(z)), np.zeros(len(z), int))
    e_mass = e_lp = 0.0
    for r in np.nonzero(~np.asarray(finished, bool))[0]:
        kk = ref.kk
        e_mass = max(e_mass, float(np.abs(cum_i[r, :kk] / SCALE - ref.cum[r, :kk]).max() / ref.mass[r]))
        k = int(ref.kept[r])
        cols = order[r, :k]
        total = np.float32(float(int(cum_i[r, k - 1])) / SCALE)
        lp32 = (z[r, cols] - z[r].max()).astype(np.float32) - np.log(total, dtype=np.float32)
        lp64 = (z[r, cols].astype(np.float64) - ref.zmax[r]) - math.log(ref.cum[r, k - 1])
        e_lp = max(e_lp, float((np.abs(lp32 - lp64) / (1 + np.abs(lp64))).max()))
    return e_mass, e_lp
