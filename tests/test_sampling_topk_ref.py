"""tests/sampling_cases.py on the CPU: what the GPU test of the truncated sampling step relies on.

1. The float32 restatement of the step (tests/sampling_ref.py:f32_step: float32 exp, fixed-point terms summed in
   integers) meets check_step with the recorded C and C_lp on every case, the exact expectations of the tie cases
   included, and draws exactly what the rule draws.
2. In every general case the band of rule 1 admits ONE kept size in EVERY unfinished row, the rule's own: the rule pins
   the kept set.
3. The worst errors of the restatement against float64 over the table are E_MASS = 3.874e-8 (prefix masses / M) and
   E_LP = 9.901e-8 (logprob / (1 + |lp|)); C and C_lp are about ten times those.  The test fails when the table no
   longer gives values in [3.6e-8, 4.1e-8] and [9.3e-8, 1.05e-7].
4. With top_k = 0, top_p = 1 and inv_temperature = 1 the restated draw is argmax(x + gumbel_noise)."""
import numpy as np
import pytest

from oracle.nm_oracle import gumbel_noise

from . import sampling_cases as SC
from . import sampling_ref as SR

EVERY = [c.name for c in SC.CASES]
GENERAL = [c.name for c in SC.GENERAL]


def _f32(b):
    c = b.case
    return SR.f32_step(b.x[:, :c.v], np.float32(c.inv_t), c.top_k, c.top_p, c.salt, SC.END, b.finished, b.lps, b.lens)


def test_table_covers_what_the_issue_names():
    assert {c.v for c in SC.GENERAL} == {1, 7, 255, 256, 257, 1001, 8193, 32000, SC.LDS_MAX + 1}
    assert all(3 <= c.rows <= 37 for c in SC.GENERAL) and {c.rows for c in SC.GENERAL} >= {3, 37}
    assert all(c.pad == 3 for c in SC.GENERAL if c.v == 1001)
    assert all(c.rows == 16 for c in SC.GENERAL if c.v == 32000)
    assert all(c.rows == 4 for c in SC.GENERAL if c.v == SC.LDS_MAX + 1)
    ks = {("V" if c.top_k == c.v else "V+5" if c.top_k == c.v + 5 else c.top_k) for c in SC.GENERAL if c.v > 1}
    assert ks >= {0, 1, 2, 40, "V", "V+5"}
    assert {c.top_p for c in SC.GENERAL} == {1.0, 0.9, 0.5, 1e-6}
    assert {c.inv_t for c in SC.GENERAL} == {1.0, 1 / 0.7, 1 / 2.5}
    assert any(SC.build(n).finished.any() for n in GENERAL)


@pytest.mark.parametrize("name", EVERY)
def test_float32_restatement_meets_the_rule(name):
    b = SC.build(name)
    errors, hits, live = SR.check_step(b.ref, _f32(b), SC.C, SC.C_LP, b.exact)
    assert errors == []
    assert hits == live == int((b.finished == 0).sum())


@pytest.mark.parametrize("name", GENERAL)
def test_general_cases_pin_the_kept_set_in_every_row(name):
    b = SC.build(name)
    got = _f32(b)
    for r in np.nonzero(b.finished == 0)[0]:
        assert SR.admissible(b.ref, r, SC.C) == [int(b.ref.kept[r])], r
        assert got.kept[r] == b.ref.kept[r]


def test_tie_cases_have_their_exact_expectations():
    b = SC.build("t_uniform_v8_p05")
    assert (b.ref.kept == 4).all()                      # terms and sums are exact binary fractions
    b = SC.build("t_uniform_v300_k5")
    assert (b.ref.order[:, :5] == np.arange(5)).all()
    b = SC.build("t_unk_columns_p_almost_1")
    assert (b.ref.kept <= b.case.v - 3).all()
    b = SC.build("t_argmax_alone")
    got = _f32(b)
    live = b.finished == 0
    assert (got.symbol[live] == b.x[:, :b.case.v].argmax(1)[live]).all() and (got.logprob[live] == 0).all()


def test_measured_float32_error_and_the_constants():
    e_mass = e_lp = 0.0
    for c in SC.CASES:
        b = SC.build(c.name)
        m, lp = SR.f32_errors(b.x[:, :c.v], np.float32(c.inv_t), c.top_k, c.top_p, b.finished)
        e_mass, e_lp = max(e_mass, m), max(e_lp, lp)
    print("float32 restatement over the sampling table: mass error {:.3e} (C = {:.3e}), logprob error {:.3e} "
          "(C_lp = {:.3e})".format(e_mass, SC.C, e_lp, SC.C_LP))
    assert 3.6e-8 <= e_mass <= 4.1e-8, e_mass
    assert 9.3e-8 <= e_lp <= 1.05e-7, e_lp
    assert (SC.E_MASS, SC.E_LP, SC.C, SC.C_LP) == (3.874e-8, 9.901e-8, 4.0e-7, 1.0e-6)


@pytest.mark.parametrize("rows,vocab,salt", [(5, 7, 0), (37, 1000, 12345), (16, 32000, 0xFFFFFFFF)])
def test_untruncated_restated_draw_is_the_gumbel_argmax(rows, vocab, salt):
    x = (np.random.RandomState(rows).randn(rows, vocab) * 2).astype(np.float32)
    zeros = np.zeros(rows, np.int32)
    got = SR.f32_step(x, np.float32(1.0), 0, 1.0, salt, SC.END, zeros, np.zeros(rows, np.float32), zeros)
    assert np.array_equal(got.symbol, (x + gumbel_noise(rows, vocab, salt)).argmax(1))
    assert (got.kept == vocab).all()
