"""nm_mbr_pairwise and nm_mbr_select (csrc/nm_mbr.hip, include/nmhip_mbr.h) on the MI355X against the host oracle of
tests/mbr_ref.py and against what the reference's own functions returned (tests/golden/mbr/pairwise.npz), on the case
table of tests/mbr_ref.py: one sample, a window of four that does not fit, an odd pair count, more positions than lanes,
more sentences than lanes, n = 64, T = 1 with empty samples, and the hand-made columns.

Tolerances, as for the reward kernels: the kernel counts in integers and finishes in double, rounding once to float.
GLEU is a quotient of two integers, correctly rounded on both sides: bit-equal.  BLEU goes through double ``pow`` and
``exp``, whose last double bit may differ between the device's library and the host's; before the one rounding to float
that moves the result by at most one float32 unit in the last place, and an exact zero (no unigram) stays one.
nm_mbr_select repeats the oracle's double additions in the oracle's order: bit-equal, on any utilities.  For GLEU the
choice must also be the ORACLE'S choice: at most 64 float32 utilities in [0, 1] sum exactly in double, so the sums
do not depend on the order, and bit-equal utilities give equal sums."""
import os

import numpy as np
import pytest
import torch

from . import mbr_ref as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "mbr", "pairwise.npz")
NAMES = list(M.cases())


@pytest.fixture(scope="module")
def golden():
    return np.load(FIXTURE)


def on_device(kind, tok, extra_stride=0):
    """(U, expected, best, chosen) as NumPy arrays; ``extra_stride`` widens the rows of the token array."""
    from neuralmonkey_amd import ops
    steps, bsz, n = tok.shape
    dev = "cuda:0"
    if extra_stride:
        wide = torch.full((steps, bsz * n + extra_stride), M.END, dtype=torch.int32, device=dev)
        wide[:, :bsz * n] = torch.tensor(tok.reshape(steps, bsz * n), device=dev)
        t = wide.as_strided((steps, bsz, n), (bsz * n + extra_stride, n, 1))
        assert not t.is_contiguous() or steps == 1
    else:
        t = torch.tensor(np.ascontiguousarray(tok), device=dev)
    utilities = ops.mbr_pairwise(kind, t, M.END)
    expected, best, chosen = ops.mbr_select(utilities, t)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (utilities, expected, best, chosen))


def check(name, golden, extra_stride=0):
    tok = M.cases()[name]
    for kind in M.KINDS:
        want = M.oracle(name, kind)
        utilities, expected, best, chosen = on_device(kind, tok, extra_stride)
        assert utilities.dtype == np.float32 and utilities.shape == want.utilities.shape
        if kind == "gleu":
            assert np.array_equal(utilities, want.utilities)
            ok = golden[name + "/gleu_defined"]
            assert np.array_equal(utilities[ok], golden[name + "/gleu"][ok]) and np.all(utilities[~ok] == 0.0)
            assert np.array_equal(utilities, utilities.transpose(0, 2, 1))
        else:
            worst = int(M.ulps(utilities, want.utilities).max())
            print(name, "BLEU ulps vs NumPy", worst, "vs reference", int(M.ulps(utilities, golden[name + "/bleu"]).max()),
                  "nonzero", int((utilities > 0).sum()), "of", utilities.size)
            assert worst <= 1 and M.ulps(utilities, golden[name + "/bleu"]).max() <= 1
            assert np.array_equal(utilities == 0, want.utilities == 0)               # an exact zero stays one
        # the select step on the device's own utilities: bit-equal to the oracle's select step on them
        own_expected, own_best, own_chosen, _ = M.select(utilities, tok)
        assert expected.tobytes() == own_expected.tobytes()
        assert np.array_equal(best, own_best) and best.dtype == np.int32
        assert np.array_equal(chosen, own_chosen) and chosen.dtype == np.int32 and chosen.shape == tok.shape[:2]
        if kind == "gleu":
            assert np.array_equal(best, want.best) and np.array_equal(chosen, want.chosen)
            assert expected.tobytes() == want.expected.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_pairwise_and_select_match_the_oracle_and_the_reference(dev, golden, name):
    check(name, golden)


def test_a_row_stride_of_its_own(dev, golden):
    check("b5_n3_t7_w4", golden, extra_stride=11)
    check("hand_made", golden, extra_stride=1)


def test_what_the_cases_are_there_for_on_the_device(dev):
    _, expected, best, chosen = on_device("gleu", M.cases()["b1_n1_t1_w3"])
    assert best.tolist() == [0] and np.array_equal(chosen, M.cases()["b1_n1_t1_w3"][:, :, 0])
    _, _, best, _ = on_device("gleu", M.cases()["b1_n2_t3_w3"])
    assert best.tolist() == [0]                                          # the tie goes to the lowest index
    utilities, expected, best, _ = on_device("gleu", M.cases()["hand_empty"])
    assert not utilities[0].any() and not expected[0].any() and best.tolist() == [0, 1]
    for kind in M.KINDS:
        _, _, best, _ = on_device(kind, M.cases()["hand_made"])
        assert best[0] == 0 and best[2] == 0 and best[3] == 1            # identical samples; the outlier loses


def same_floats(a, b):
    """Bit-equal where there is a number, NaN where there is NaN."""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


def select_on_device(utilities, tok):
    from neuralmonkey_amd import ops
    dev = "cuda:0"
    out = ops.mbr_select(torch.tensor(utilities, device=dev), torch.tensor(tok, device=dev))
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


def test_select_on_hand_made_utilities(dev):
    nan = np.nan
    utilities = np.asarray([
        [[0.5, 0.5, 0.0], [0.25, 0.25, 0.5], [0.125, 0.0, 0.0]],             # top tie of rows 0 and 1: 0
        [[-3.0, -1.0, -1.0], [-1.0, -1.0, -1.0], [-2.0, -0.5, -0.5]],         # negative values, a tie of rows 1 and 2: 1
        [[nan, 1.0, 1.0], [0.0, 0.25, 0.0], [0.0, 0.0, 0.125]],               # a NaN row sorts behind everything: 1
        [[nan, 0.0, 0.0], [0.0, nan, 0.0], [0.0, 0.0, nan]],                  # an all-NaN sentence: 0
        [[0.1, 0.2, 0.3], [0.3, 0.2, 0.1], [1e-8, 0.6, 1e-8]],                # sums that depend on the order of addition
    ], np.float32)
    tok = np.arange(2 * 5 * 3, dtype=np.int32).reshape(2, 5, 3)
    expected, best, chosen = select_on_device(utilities, tok)
    want_expected, want_best, want_chosen, _ = M.select(utilities, tok)
    assert want_best.tolist()[:4] == [0, 1, 1, 0]
    assert same_floats(expected, want_expected) and np.isnan(expected[3]).all() and np.isnan(expected[2, 0])
    assert np.array_equal(best, want_best) and np.array_equal(chosen, want_chosen)
    # n = 1: whatever the utility is, the one sample is chosen
    for value in (0.75, -2.0, nan):
        one = np.full((4, 1, 1), value, np.float32)
        tok1 = np.arange(3 * 4, dtype=np.int32).reshape(3, 4, 1)
        expected, best, chosen = select_on_device(one, tok1)
        assert best.tolist() == [0, 0, 0, 0] and np.array_equal(chosen, tok1[:, :, 0])
        assert same_floats(expected, one[:, :, 0])
    # n = 64 with random utilities of both signs, more sentences than lanes
    rng = np.random.default_rng(11)
    many = (rng.standard_normal((67, 64, 64)) * 3).astype(np.float32)
    many[5, 9] = many[5, 40]                                               # an exact tie somewhere
    tok64 = rng.integers(0, 50, (5, 67, 64)).astype(np.int32)
    expected, best, chosen = select_on_device(many, tok64)
    want_expected, want_best, want_chosen, _ = M.select(many, tok64)
    assert expected.tobytes() == want_expected.tobytes()
    assert np.array_equal(best, want_best) and np.array_equal(chosen, want_chosen)


def test_two_runs_are_bit_equal(dev):
    tok = M.cases()["b3_n17_t70_w5"]
    for kind in M.KINDS:
        first, second = on_device(kind, tok), on_device(kind, tok)
        for a, b in zip(first, second):
            assert a.tobytes() == b.tobytes()
