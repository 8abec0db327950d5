"""tests/beam_wide_cases.py on the CPU: what the GPU test of the wide beam step relies on.

1. The float32 restatement of the beam body (oracle/beam_ref.py:f32_step_outputs), with its lse moved by -2 / 0 / +2
   ulp, meets check_step with C = tests.beam_cases.C on every case, the exact expectation of the tie cases included.
2. In every general case (and its k = 16 twin) the band at the boundary holds the k-th candidate alone in EVERY
   sentence, so the rule pins the selected set.
3. The worst |float32 restatement - float64| / (1 + |score|) over the table is 2.62e-7: C is 13 times that.  The test
   fails when the table no longer gives a value in [2.3e-7, 2.7e-7]."""
import numpy as np
import pytest

from oracle import beam_ref as R

from . import beam_wide_cases as WC

EVERY = [c.name for c in WC.CASES + WC.K16]
GENERAL = [c.name for c in WC.GENERAL + WC.K16]
TIES = [c.name for c in WC.CASES if not c.general]


def _f32(o, ulps=0):
    c = o.case
    return R.f32_step_outputs(o.logits, c.k, o.lps, o.lens, o.fin, o.penalty, c.end, o.rmax, o.rlse, ulps)


def test_table_is_the_one_the_kernel_test_names():
    assert len(WC.CASES) == 21 and len(WC.GENERAL) == 10 and len(WC.K16) == 10
    assert {c.k for c in WC.CASES} >= {17, 20, 24, 32, 33, 40, 48, 64}
    assert all(16 < c.k <= 64 for c in WC.CASES) and all(c.k == 16 for c in WC.K16)
    o = WC.build("w_k64_v32000")
    assert o.logits.shape == (128, 32000)
    assert WC.build("w_k24_v300_ens").case.ensemble and (WC.build("w_k24_v300_ens").logits <= 0).all()
    # V < k on a first step: 24 picks come out of the tie at -1e9, beam 1's lowest words
    o = WC.build("t_first_step_spill_k64_v40")
    assert (np.sort(o.exact[:, :40], axis=1) == np.arange(40)).all() and (o.exact[:, 40:] == np.arange(40, 64)).all()


@pytest.mark.parametrize("name", EVERY)
def test_float32_restatement_meets_the_rule(name):
    o = WC.build(name)
    for ulps in (0, 2, -2):
        assert R.check_step(o.ref, _f32(o, ulps), WC.C, o.exact) == [], ulps


@pytest.mark.parametrize("name", GENERAL)
def test_general_cases_pin_the_selected_set_in_every_sentence(name):
    o = WC.build(name)
    n = [cnt for _, cnt in R.boundary(o.ref, WC.C)]
    assert n == [1] * o.case.b, n
    got = _f32(o)
    want = R.stable_topk(o.ref.scores, o.case.k)
    for s in range(o.case.b):
        assert set((got["beam"][s] * o.case.v + got["word"][s]).tolist()) == set(want[s].tolist())


def test_measured_float32_error_and_the_constant():
    worst = 0.0
    for c in WC.CASES:
        o = WC.build(c.name)
        for ulps in (0, 2, -2):
            sc = R.beam_step_f32(o.logits, c.k, o.lps, o.lens, o.fin, o.penalty, c.end, o.rmax, o.rlse, ulps)[0]
            worst = max(worst, float((np.abs(sc - o.ref.scores) / (1 + np.abs(o.ref.scores))).max()))
    print("float32 restatement error over the wide table: {:.3e}; C = {:.3e}".format(worst, WC.C))
    assert 2.3e-7 <= worst <= 2.7e-7, worst
    assert WC.C == 3.52e-6


@pytest.mark.parametrize("name", TIES)
def test_first_step_rows_of_the_tie_cases_round_to_the_same_sum(name):
    o = WC.build(name)
    assert R.first_step_logprob_bound(o.ref) < 30.0
