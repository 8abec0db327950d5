"""Float64 restatement of one beam-search body (decoders/beam_search_decoder.py:440-501) and the acceptance rule the
beam step kernels of csrc/nm_logits.hip are held to (tests/test_beam_ref.py on the CPU, tests/test_beam_kernels_gpu.py
on the GPU).  NumPy only.

  beam_step_ref64   the expected values: log-softmax of the float32 logits in float64, the finished row [0, -1e9, ...],
                    + logprob_sum, / penalty[lengths + 1 - finished]
  beam_step_f32     the same arithmetic in float32 in the kernels' operation order (lps + ((x - max) - lse)) / pen: the
                    yardstick the bound C is derived from -- never an expected value
  tile_stats        the {max, sum exp(x - max), first argmax, 0} records nm_logits_stats_gemm documents, for either
                    tile width, so that nm_beam_topk_step_tiles can be driven without the GEMM
  check_step        the acceptance rule; returns the list of problems it found
"""
import numpy as np

NEG = -1e9                                   # the reference's INF (beam_search_decoder.py:42), with its sign


class BeamRef:
    """What beam_step_ref64 returns; unpacks as (scores, hyp, state, (rmax, rlse))."""

    def __init__(self, scores, hyp, rmax, rlse, k, v, lengths, finished, end_id, logprob_sum, pen):
        self.scores, self.hyp, self.rmax, self.rlse, self.pen = scores, hyp, rmax, rlse, pen
        self.b, self.k, self.v = scores.shape[0], k, v
        self.lengths, self.finished, self.end_id, self.logprob_sum = lengths, finished, end_id, logprob_sum

    def state(self, flat):
        """Derived search state of flat candidates [B, n]: (beam, word, length, finished, source row)."""
        flat = np.asarray(flat, np.int64)
        beam, word = flat // self.v, flat % self.v
        bi = np.arange(self.b)[:, None]
        fin = self.finished[bi, beam]
        return (beam, word, self.lengths[bi, beam] + 1 - fin.astype(np.int64), fin | (word == self.end_id),
                bi * self.k + beam)

    def __iter__(self):
        return iter((self.scores, self.hyp, self.state, (self.rmax, self.rlse)))


def _shape(logits, k, logprob_sum, lengths, finished):
    logits = np.asarray(logits)
    assert logits.dtype == np.float32 and logits.ndim == 2 and logits.shape[0] % k == 0
    b, v = logits.shape[0] // k, logits.shape[1]
    lps = np.asarray(logprob_sum, np.float32).reshape(b, k)
    return logits, b, v, lps, np.asarray(lengths, np.int64).reshape(b, k), np.asarray(finished, bool).reshape(b, k)


def row_stats64(logits):
    """(float32 row maximum, float64 log sum exp(x - max)) of float32 rows."""
    x = np.asarray(logits, np.float32)
    mx = x.max(1)
    x64 = x.astype(np.float64)
    return mx, np.log(np.exp(x64 - mx.astype(np.float64)[:, None]).sum(1))


def beam_step_ref64(logits, k, logprob_sum, lengths, finished, penalty, end_id, rmax=None, rlse=None):
    """One beam body in float64 over float32 inputs.  ``rmax`` / ``rlse`` replace the row statistics (the ensemble
    convention: the logits are log-probabilities and both statistics are zero)."""
    logits, b, v, lps, lens, fin = _shape(logits, k, logprob_sum, lengths, finished)
    if rmax is None:
        mx, lse = row_stats64(logits)
    else:
        mx, lse = np.asarray(rmax, np.float32).reshape(-1), np.asarray(rlse, np.float32).reshape(-1).astype(np.float64)
    lp = (logits.astype(np.float64) - mx.astype(np.float64)[:, None]) - lse[:, None]
    fin_row = np.full(v, NEG, np.float64)
    fin_row[0] = 0.0
    lp = np.where(fin.reshape(-1, 1), fin_row[None, :], lp).reshape(b, k, v)
    hyp = lps.astype(np.float64)[:, :, None] + lp
    hl = lens + 1 - fin.astype(np.int64)
    pen = np.asarray(penalty, np.float32).astype(np.float64)[hl]
    scores = (hyp / pen[:, :, None]).reshape(b, k * v)
    return BeamRef(scores, hyp.reshape(b, k * v), mx, lse, k, v, lens, fin, int(end_id), lps, pen)


def shift_ulps(x, n):
    x = np.asarray(x, np.float32).copy()
    for _ in range(abs(int(n))):
        x = np.nextafter(x, np.float32(np.inf if n > 0 else -np.inf))
    return x


def beam_step_f32(logits, k, logprob_sum, lengths, finished, penalty, end_id, rmax=None, rlse=None, lse_ulps=0):
    """(scores, hyp, rmax, rlse), all float32, in the kernels' operation order.  The lse is the float64 value rounded
    to float32 and moved by ``lse_ulps``, which stands in for the kernels' different float32 summation orders."""
    logits, b, v, lps, lens, fin = _shape(logits, k, logprob_sum, lengths, finished)
    if rmax is None:
        mx, lse64 = row_stats64(logits)
        lse = shift_ulps(lse64.astype(np.float32), lse_ulps)
    else:
        mx, lse = np.asarray(rmax, np.float32).reshape(-1), np.asarray(rlse, np.float32).reshape(-1)
    lp = ((logits - mx[:, None]).astype(np.float32) - lse[:, None]).astype(np.float32)
    fin_row = np.full(v, NEG, np.float32)
    fin_row[0] = 0.0
    lp = np.where(fin.reshape(-1, 1), fin_row[None, :], lp).reshape(b, k, v)
    hyp = (lps[:, :, None] + lp).astype(np.float32)
    pen = np.asarray(penalty, np.float32)[lens + 1 - fin.astype(np.int64)]
    scores = (hyp / pen[:, :, None]).astype(np.float32)
    return scores.reshape(b, k * v), hyp.reshape(b, k * v), mx, lse


def stable_topk(scores, k):
    """Flat indices [B, k] of the k largest values, exact equality resolved to the lower index (tf.nn.top_k)."""
    out = np.empty((scores.shape[0], k), np.int64)
    for b, s in enumerate(scores):
        n = s.shape[0]
        if n > 4 * k:
            keep = np.nonzero(s >= np.partition(s, n - k)[n - k])[0]
        else:
            keep = np.arange(n)
        out[b] = keep[np.argsort(-s[keep], kind="stable")[:k]]
    return out


def f32_step_outputs(logits, k, logprob_sum, lengths, finished, penalty, end_id, rmax=None, rlse=None, lse_ulps=0):
    """The float32 restatement with its stable top-k, in the layout of a kernel's outputs (what check_step takes)."""
    sc, hyp, mx, lse = beam_step_f32(logits, k, logprob_sum, lengths, finished, penalty, end_id, rmax, rlse, lse_ulps)
    logits, b, v, lps, lens, fin = _shape(logits, k, logprob_sum, lengths, finished)
    idx = stable_topk(sc, k)
    bi = np.arange(b)[:, None]
    beam, word = idx // v, idx % v
    nf = fin[bi, beam] | (word == end_id)
    return {"score": sc[bi, idx], "word": word, "beam": beam, "logprob_sum": hyp[bi, idx],
            "lengths": lens[bi, beam] + 1 - fin[bi, beam], "finished": nf.astype(np.int32), "src_row": bi * k + beam,
            "rmax": mx, "rlse": lse, "all_finished": int(nf.all()), "all_finished_from0": 0}


def exact_selection(ref):
    """Structural-tie cases: the float64 scores with exact equality resolved to the lower flat index.  A first-step
    row (logprob_sum = -1e9) takes the rounded sum: float32(-1e9 + lp) is exactly -1e9 while |lp| < 30, whatever the
    last bits of a kernel's lse, so all its candidates tie."""
    first = (ref.logprob_sum <= np.float32(-1e8)) & ~ref.finished                          # [B, k]
    s = ref.scores.reshape(ref.b, ref.k, ref.v).copy()
    for b, j in zip(*np.nonzero(first)):
        s[b, j, :] = NEG / ref.pen[b, j]
    return stable_topk(s.reshape(ref.b, -1), ref.k)


def first_step_logprob_bound(ref):
    """Largest |log-probability| in the first-step rows (the rounded-sum rule needs it below 30)."""
    first = (ref.logprob_sum <= np.float32(-1e8)) & ~ref.finished
    if not first.any():
        return 0.0
    lp = ref.hyp.reshape(ref.b, ref.k, ref.v) - ref.logprob_sum.astype(np.float64)[:, :, None]
    return float(np.abs(lp[first]).max())


def tile_stats(logits, tile_w):
    """[rows, ntiles, 4] float32 records {max, sum exp(x - max), first argmax (global column, int32 bits), 0} of every
    ``tile_w``-column tile, computed in float64 and rounded; a partial last tile covers its valid columns only."""
    x = np.asarray(logits, np.float32)
    rows, v = x.shape
    nt = (v + tile_w - 1) // tile_w
    out = np.zeros((rows, nt, 4), np.float32)
    arg = np.zeros((rows, nt), np.int32)
    for t in range(nt):
        seg = x[:, t * tile_w:min(v, (t + 1) * tile_w)]
        mx = seg.max(1)
        out[:, t, 0] = mx
        out[:, t, 1] = np.exp(seg.astype(np.float64) - mx.astype(np.float64)[:, None]).sum(1).astype(np.float32)
        arg[:, t] = seg.argmax(1) + t * tile_w
    out[:, :, 2] = arg.view(np.float32)
    return out


def merge_tile_stats(stats):
    """(max, first argmax, float64 lse) of every row from its tile records."""
    mx = stats[:, :, 0]
    arg = np.ascontiguousarray(stats[:, :, 2]).view(np.int32)
    big = mx.max(1)
    first = np.where(mx == big[:, None], arg, np.iinfo(np.int32).max).min(1)
    sm = stats[:, :, 1].astype(np.float64) * np.exp(mx.astype(np.float64) - big.astype(np.float64)[:, None])
    return big, first, np.log(sm.sum(1))


def boundary(ref, bound):
    """Per sentence: (S_k, number of candidates neither forced in nor forced out by the rule).  A sentence whose band
    holds the k-th candidate alone has its selected SET pinned exactly."""
    out = []
    for s in ref.scores:
        n = s.shape[0]
        sk = np.partition(s, n - ref.k)[n - ref.k]
        tk = bound * (1.0 + abs(sk))
        tol = bound * (1.0 + np.abs(s))
        inside = ~(s - tol > sk + tk) & ~(s + tol < sk - tk)
        out.append((float(sk), int(inside.sum())))
    return out


def check_step(ref, got, bound, exact=None):
    """The acceptance rule of one beam step.  ``got``: score, word, beam, logprob_sum, lengths, finished, src_row
    [B, k]; rmax, rlse [B*k] (optional: a kernel that takes them as inputs has none); all_finished (preset 1) and
    all_finished_from0 (preset 0).  ``exact`` [B, k]: the expected flat indices of a structural-tie case."""
    p = []
    b, k, v = ref.b, ref.k, ref.v
    g = {n: np.asarray(a) for n, a in got.items()}
    for n in ("score", "word", "beam", "logprob_sum", "lengths", "finished", "src_row"):
        if g[n].shape != (b, k):
            return ["{}: shape {} instead of {}".format(n, g[n].shape, (b, k))]
    word, beam = g["word"].astype(np.int64), g["beam"].astype(np.int64)
    if ((word < 0) | (word >= v) | (beam < 0) | (beam >= k)).any():
        return ["beam / word out of range: beam {} word {}".format(beam.tolist(), word.tolist())]
    flat = beam * v + word
    score = g["score"].astype(np.float64)
    if not np.isfinite(score).all():
        p.append("non-finite out_score")
    for s in range(b):
        S = ref.scores[s]
        n = S.shape[0]
        if len(set(flat[s].tolist())) != k:
            p.append("sentence {}: indices not distinct {}".format(s, flat[s].tolist()))
            continue
        sk = np.partition(S, n - k)[n - k]
        tk = bound * (1.0 + abs(sk))
        tol = bound * (1.0 + np.abs(S))
        mine = flat[s]
        err = np.abs(score[s] - S[mine])
        if (err > tol[mine]).any():
            i = int(np.argmax(err - tol[mine]))
            p.append("sentence {}: out_score[{}] = {!r}, float64 {!r} at flat {}".format(s, i, score[s, i], S[mine[i]],
                                                                                        mine[i]))
        d = np.diff(g["score"][s])
        if (d > 0).any():
            p.append("sentence {}: out_score increases at {}".format(s, np.nonzero(d > 0)[0].tolist()))
        if ((d == 0) & (np.diff(mine) <= 0)).any():
            p.append("sentence {}: equal scores with descending flat indices {}".format(s, mine.tolist()))
        must = np.nonzero(S - tol > sk + tk)[0]
        missing = np.setdiff1d(must, mine)
        if missing.size:
            p.append("sentence {}: candidates {} score above the band and are not returned".format(s, missing[:8].tolist()))
        low = S[mine] + tol[mine] < sk - tk
        if low.any():
            p.append("sentence {}: returned {} score below the band".format(s, mine[low].tolist()))
    rb, rw, rl, rf, rs = ref.state(flat)
    for name, want in (("lengths", rl), ("finished", rf.astype(np.int64)), ("src_row", rs)):
        if not np.array_equal(g[name].astype(np.int64), want):
            p.append("{}: {} instead of {}".format(name, g[name].tolist(), want.tolist()))
    hyp = ref.hyp[np.arange(b)[:, None], flat]
    bad = np.abs(g["logprob_sum"].astype(np.float64) - hyp) > bound * (1.0 + np.abs(hyp))
    if bad.any() or not np.isfinite(g["logprob_sum"]).all():
        p.append("logprob_sum: {} instead of {}".format(g["logprob_sum"][bad].tolist(), hyp[bad].tolist()))
    live = ~ref.finished.reshape(-1)
    if "rmax" in g:
        if not np.array_equal(g["rmax"].reshape(-1)[live], ref.rmax[live]):
            p.append("rmax differs from the float32 row maximum in live rows")
        lse = g["rlse"].reshape(-1).astype(np.float64)[live]
        if not (np.abs(lse - ref.rlse[live]) <= bound * (1.0 + np.abs(ref.rlse[live]))).all():
            p.append("rlse: {} instead of {}".format(lse.tolist()[:4], ref.rlse[live].tolist()[:4]))
    want_all = int(bool((g["finished"] != 0).all()))
    if int(g["all_finished"]) != want_all:
        p.append("all_finished preset to 1 ended as {}, the outputs say {}".format(int(g["all_finished"]), want_all))
    if int(g["all_finished_from0"]) != 0:
        p.append("all_finished preset to 0 ended as {}".format(int(g["all_finished_from0"])))
    if exact is not None and not np.array_equal(flat, exact):
        p.append("structural ties: picked {} instead of {}".format(flat.tolist(), np.asarray(exact).tolist()))
    return p
