"""oracle/beam_ref.py and tests/beam_cases.py on the CPU: the float64 restatement of the beam body reproduces what the
reference's own BeamSearchDecoder produced (tests/golden/ref_exec/beam_body*.npz) and agrees with the float32 oracle of
test_kernels_gpu.py; tile_stats merges back to plain max / argmax / lse; a float32 evaluation in the kernels'
operation order meets the acceptance rule on every case of the table, also with its lse moved by +-2 ulp (headroom);
the general cases pin the selected set (sharpness); and check_step rejects planted errors.

Measured float32 restatement error over the table: 2.13e-7 relative to 1 + |score| (beam_cases.MEASURED_F32_ERROR =
2.2e-7 bounds it); C = 16 x 2.2e-7 = 3.52e-6, below the cap of 1e-5."""
import json
import os

import numpy as np
import pytest

from oracle import beam_ref as R
from oracle import nm_oracle as O

from . import beam_cases as BC

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_exec")
EVERY = [c.name for c in BC.CASES] + [BC.GEMM_CASE.name]
GENERAL = [n for n in EVERY if BC.BY_NAME[n].general]
TIES = [n for n in EVERY if not BC.BY_NAME[n].general]


def _f32(o, ulps=0):
    c = o.case
    return R.f32_step_outputs(o.logits, c.k, o.lps, o.lens, o.fin, o.penalty, c.end, o.rmax, o.rlse, ulps)


@pytest.mark.parametrize("case", ["beam_body", "beam_body_k5_alpha0", "beam_body_k4_alpha1"])
def test_restatement_reproduces_the_reference_executed_search(case):
    """Whole searches of the reference's BeamSearchDecoder over a logits table, stepped with beam_step_ref64."""
    z = np.load(os.path.join(FIX, case + ".npz"))
    cfg = json.loads(str(z["cfg"]))
    table = z["in/table"]
    k, max_steps, alpha = cfg["beam"]
    b, v = cfg["batch"], cfg["vocab"]
    pen = z["out/length_penalty"]                                     # the reference's own _length_penalty values
    assert np.array_equal(pen, O.length_penalty(np.arange(12), alpha, np.float32))
    sent = np.repeat(np.arange(b), k)
    logits = table[sent, 0, O.START]
    tokens = logits.argmax(1).reshape(1, b, k)
    lps = np.tile(np.array([0.0] + [-1e9] * (k - 1), np.float32), (b, 1))
    lens, fin = np.zeros((b, k), np.int64), np.zeros((b, k), bool)
    scores = np.zeros((b, k))
    bi = np.arange(b)[:, None]
    step = 1
    while step - 1 < max_steps and not fin.all():
        ref = R.beam_step_ref64(logits, k, lps, lens, fin, pen, O.END)
        s, hyp, state, (mx, lse) = ref
        assert np.array_equal(mx, logits.max(1))
        idx = R.exact_selection(ref)
        beam, word, lens, fin, src = state(idx)
        scores, lps = s[bi, idx], hyp[bi, idx].astype(np.float32)
        tokens = np.concatenate([tokens[:, bi, beam], word[None]], axis=0)
        logits = table[sent, step, word.reshape(-1)]
        step += 1
    assert step == int(z["out/dec_step"])
    assert np.array_equal(tokens, z["out/token_ids"])
    assert np.array_equal(lens, z["out/lengths"]) and np.array_equal(fin, z["out/finished"])
    assert np.abs(scores - z["out/scores"]).max() <= 2e-6 * max(1.0, np.abs(z["out/scores"]).max())
    want = z["out/logprob_sum"].astype(np.float64)
    assert (np.abs(lps - want) <= 2e-6 * np.maximum(1.0, np.abs(want))).all()


@pytest.mark.parametrize("b,k,v,alpha", [(3, 3, 70, 0.6), (1, 2, 17, 1.0), (2, 10, 37, 0.0), (4, 5, 516, 0.6)])
def test_restatement_agrees_with_the_float32_oracle_of_the_two_pass_test(b, k, v, alpha):
    from .test_kernels_gpu import _beam_step_ref
    rng = np.random.default_rng(b + k + v)
    logits = (rng.standard_normal((b * k, v)) * 4).astype(np.float32)
    lps = (-rng.random((b, k)) * 20).astype(np.float32)
    lens = rng.integers(0, 30, size=(b, k)).astype(np.int32)
    fin = rng.random((b, k)) < 0.3
    fin[0] = True
    sc, hyp, hl, ts, ti = _beam_step_ref(logits, k, lps, lens, fin, alpha)
    ref = R.beam_step_ref64(logits, k, lps, lens, fin, BC.penalty_table(alpha), O.END)
    assert (np.abs(sc - ref.scores) <= BC.C * (1 + np.abs(ref.scores))).all()
    assert (np.abs(hyp - ref.hyp) <= BC.C * (1 + np.abs(ref.hyp))).all()
    beam, word, length, nf, src = ref.state(ti[:, :k])
    bi = np.arange(b)[:, None]
    assert np.array_equal(length, hl[bi, beam])
    assert np.array_equal(nf, fin[bi, beam] | (ti[:, :k] % v == O.END)) and np.array_equal(src, bi * k + ti[:, :k] // v)
    # the same arithmetic in float32, in the kernels' operation order, is the oracle's
    s32 = R.beam_step_f32(logits, k, lps, lens, fin, BC.penalty_table(alpha), O.END)[0]
    assert (np.abs(s32 - sc) <= 4 * np.spacing(np.abs(sc))).all()


@pytest.mark.parametrize("v,w", [(64, 64), (68, 64), (132, 128), (260, 128), (1000, 64), (1000, 128), (5, 128)])
def test_tile_stats_merge_back_to_the_row_statistics(v, w):
    rng = np.random.default_rng(v + w)
    x = (rng.standard_normal((7, v)) * 3).astype(np.float32)
    x[0, [1 % v, v - 1]] = 20.0                                        # equal maxima in two tiles: the first wins
    x[1, :] = -2.5
    st = R.tile_stats(x, w)
    assert st.shape == (7, (v + w - 1) // w, 4) and st.dtype == np.float32 and (st[:, :, 3] == 0).all()
    mx, arg, lse = R.merge_tile_stats(st)
    assert np.array_equal(mx, x.max(1)) and np.array_equal(arg, x.argmax(1))
    want = R.row_stats64(x)[1]
    assert np.abs(lse - want).max() < 1e-6
    args = np.ascontiguousarray(st[:, :, 2]).view(np.int32)          # global columns, inside their own tile
    lo = np.arange(st.shape[1]) * w
    assert ((args >= lo) & (args < np.minimum(lo + w, v))).all()


def test_measured_float32_error_and_the_constant():
    worst = 0.0
    for name in EVERY:
        o = BC.build(name)
        c = o.case
        for ulps in (0, 2, -2):
            sc = R.beam_step_f32(o.logits, c.k, o.lps, o.lens, o.fin, o.penalty, c.end, o.rmax, o.rlse, ulps)[0]
            worst = max(worst, float((np.abs(sc - o.ref.scores) / (1 + np.abs(o.ref.scores))).max()))
    print("float32 restatement error over the table: {:.3e}; C = {:.3e}".format(worst, BC.C))
    assert 0.9 * BC.MEASURED_F32_ERROR <= worst <= BC.MEASURED_F32_ERROR, worst
    assert BC.C == 16 * BC.MEASURED_F32_ERROR and BC.C <= BC.C_CAP == 1e-5


@pytest.mark.parametrize("name", EVERY)
def test_headroom_the_float32_restatement_meets_the_rule(name):
    o = BC.build(name)
    for ulps in (0, 2, -2):
        assert R.check_step(o.ref, _f32(o, ulps), BC.C, o.exact) == [], ulps


def test_general_cases_pin_the_selected_set():
    """Sharpness: in >= 95% of a case's sentences the band at the boundary holds the k-th candidate alone."""
    total = sharp = 0
    for name in GENERAL:
        o = BC.build(name)
        n = [cnt for _, cnt in R.boundary(o.ref, BC.C)]
        assert all(cnt >= 1 for cnt in n)
        assert np.mean([cnt == 1 for cnt in n]) >= 0.95, (name, n)
        total, sharp = total + len(n), sharp + sum(cnt == 1 for cnt in n)
        # ... and then the rule leaves the float32 restatement no choice but the float64 selection
        got = _f32(o)
        want = R.stable_topk(o.ref.scores, o.case.k)
        for s, cnt in enumerate(n):
            if cnt == 1:
                assert set((got["beam"][s] * o.case.v + got["word"][s]).tolist()) == set(want[s].tolist())
    print("{} of {} sentences sharp".format(sharp, total))


def test_table_covers_what_it_claims():
    ks = {c.k for c in BC.CASES}
    assert ks >= {1, 2, 4, 5, 8, 9, 16}
    for kern in ("twopass", "ensemble", "fused", "tiles64", "tiles128"):
        mine = [c for c in BC.CASES if kern in c.kernels]
        assert {c.alpha for c in mine} >= {0.0, 0.6, 1.0} or kern == "ensemble"
        assert any(c.end == 2 for c in mine) and any(c.end == c.v - 1 for c in mine) or kern == "ensemble"
        assert any(c.pad == 0 for c in mine) and any(c.pad == 4 for c in mine)
        assert any(c.v < c.k for c in mine) and any(c.k == 1 for c in mine) or kern == "ensemble"
    assert {c.pad for c in BC.CASES} == {0, 3, 4}
    for c in BC.CASES + [BC.GEMM_CASE]:
        assert c.b * c.k <= 80 or c is BC.GEMM_CASE
        o = BC.build(c.name)
        assert o.lens.min() >= 0 and o.lens.max() <= BC.TABLE - 2
        if c.general and "f" not in c.roles and "e" not in c.roles:
            assert o.lps.min() >= -30 and o.lps.max() <= 0
    # new finished flags arise, all_finished takes both values, and the all-finished inputs emit <pad>
    o = BC.build("v1000_k9")
    got = _f32(o)
    assert (got["finished"].astype(bool) & ~o.fin[np.arange(o.case.b)[:, None], got["beam"]]).any()
    assert got["all_finished"] == 0
    assert _f32(BC.build("every_pick_ends"))["all_finished"] == 1
    got = _f32(BC.build("all_inputs_finished"))
    assert got["all_finished"] == 1 and (got["word"] == 0).all() and (np.diff(got["score"], axis=1) <= 0).all()
    assert sorted(got["beam"][0].tolist()) == list(range(5)) and got["beam"][0].tolist() != list(range(5))


@pytest.mark.parametrize("name", TIES)
def test_first_step_rows_of_the_tie_cases_round_to_the_same_sum(name):
    """The rounded-sum rule of exact_selection holds on the cases' own inputs: |lp| < 30 in every first-step row."""
    o = BC.build(name)
    assert R.first_step_logprob_bound(o.ref) < 30.0
    first = (o.lps == np.float32(-1e9))
    if first.any():
        hyp = R.beam_step_f32(o.logits, o.case.k, o.lps, o.lens, o.fin, o.penalty, o.case.end, lse_ulps=2)[1]
        assert (hyp.reshape(o.case.b, o.case.k, -1)[first] == np.float32(-1e9)).all()


def test_first_step_spill_goes_to_beam_one():
    o = BC.build("tie_first_step_v4_k8")
    assert (o.exact[:, 4:] == np.arange(4, 8)).all() and (np.sort(o.exact[:, :4], axis=1) == np.arange(4)).all()


# ---------------------------------------------------------------------------------------------------------------
# check_step rejects planted errors
def _planted(name="v1000_k5"):
    o = BC.build(name)
    got = {n: np.array(a) for n, a in _f32(o).items()}
    assert R.check_step(o.ref, got, BC.C, o.exact) == []
    return o, got


def _rejects(o, got, what):
    problems = R.check_step(o.ref, got, BC.C, o.exact)
    assert any(what in p for p in problems), problems


def test_checker_rejects_two_outputs_swapped():
    o, got = _planted()
    for n in ("score", "word", "beam", "logprob_sum", "lengths", "finished", "src_row"):
        got[n][2, [1, 2]] = got[n][2, [2, 1]]
    _rejects(o, got, "out_score increases")


def test_checker_rejects_a_pick_outside_the_band():
    o, got = _planted()
    s = 2
    S = o.ref.scores[s]
    order = np.argsort(-S, kind="stable")
    k, v = o.case.k, o.case.v
    assert S[order[k - 1]] - S[order[k]] > 1e-3                        # the (k+1)-th lies far outside
    flat = order[k]
    beam, word, length, fin, src = (a[s, 0] for a in o.ref.state(np.full((o.case.b, 1), flat)))
    for n in ("score", "word", "beam", "logprob_sum", "lengths", "finished", "src_row"):
        got[n][s, :-1] = got[n][s, 1:]                                  # the best pick goes, the outsider comes last
    got["beam"][s, -1], got["word"][s, -1], got["score"][s, -1] = beam, word, S[flat]
    got["lengths"][s, -1], got["finished"][s, -1], got["src_row"][s, -1] = length, fin, src
    got["logprob_sum"][s, -1] = o.ref.hyp[s, flat]
    got["all_finished"] = int(got["finished"].all())
    problems = R.check_step(o.ref, got, BC.C)
    assert any("below the band" in p for p in problems) and any("not returned" in p for p in problems), problems
    assert len(problems) == 2                                           # everything else about the pick is consistent


def test_checker_rejects_a_wrong_score_sum_and_statistics():
    o, got = _planted()
    good = {n: a.copy() for n, a in got.items()}
    got["score"][0, 0] *= np.float32(1 + 2e-5)
    _rejects(o, got, "out_score[0]")
    got = {n: a.copy() for n, a in good.items()}
    got["logprob_sum"][1, 1] += np.float32(1e-3)
    _rejects(o, got, "logprob_sum")
    live = np.nonzero(~o.fin.reshape(-1))[0][0]
    got = {n: a.copy() for n, a in good.items()}
    got["rmax"][live] = np.nextafter(got["rmax"][live], np.float32(np.inf))
    _rejects(o, got, "rmax")
    got = {n: a.copy() for n, a in good.items()}
    got["rlse"][live] += np.float32(1e-3)
    _rejects(o, got, "rlse")
    got = {n: a.copy() for n, a in good.items()}
    got["word"][0, 1], got["beam"][0, 1] = got["word"][0, 0], got["beam"][0, 0]
    _rejects(o, got, "not distinct")
    got = {n: a.copy() for n, a in good.items()}
    got["word"][0, 1] = o.case.v
    _rejects(o, got, "out of range")


def test_checker_rejects_a_wrong_finished_flag_length_and_source_row():
    o, good = _planted()
    for name, what in (("finished", "finished"), ("lengths", "lengths"), ("src_row", "src_row")):
        got = {n: a.copy() for n, a in good.items()}
        got[name][1, 0] += 1
        _rejects(o, got, what + ":")


def test_checker_rejects_a_wrong_all_finished():
    o, got = _planted()
    assert got["all_finished"] == 0
    got["all_finished"] = np.array(1)
    _rejects(o, got, "all_finished preset to 1")
    o, got = _planted("every_pick_ends")
    got["all_finished"] = np.array(0)
    _rejects(o, got, "all_finished preset to 1")
    o, got = _planted()
    got["all_finished_from0"] = np.array(1)
    _rejects(o, got, "all_finished preset to 0")
    got["all_finished_from0"] = np.array(-1)                           # an unwritten sentinel
    _rejects(o, got, "all_finished preset to 0")


def test_checker_rejects_a_tie_resolved_to_the_higher_index():
    o, got = _planted("tie_uniform_same_k5")
    assert (got["word"] == np.arange(5)).all() and (got["beam"] == 0).all()
    # inside the output: two equal scores in descending index order
    swapped = {n: a.copy() for n, a in got.items()}
    swapped["word"][0, [0, 1]] = swapped["word"][0, [1, 0]]
    _rejects(o, swapped, "equal scores with descending flat indices")
    # at the boundary: a tied candidate with a higher index instead of the k-th; only the exact expectation sees it
    higher = {n: a.copy() for n, a in got.items()}
    higher["word"][0, 4] = 7
    assert R.check_step(o.ref, higher, BC.C) == []
    _rejects(o, higher, "structural ties")
    # identical beams: the lower beam comes first
    o, got = _planted("tie_identical_rows_k4")
    assert (got["beam"] == np.arange(4)).all() and (got["word"] == got["word"][:, :1]).all()
    for n in ("beam", "src_row"):
        got[n][0, [2, 3]] = got[n][0, [3, 2]]
    _rejects(o, got, "equal scores with descending flat indices")
