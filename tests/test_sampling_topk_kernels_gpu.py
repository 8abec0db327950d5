"""nm_sample_step (temperature, top-k, nucleus; csrc/nm_sample.hip) against the float64 rule of tests/sampling_ref.py
on the case table of tests/sampling_cases.py: every case through check_step with the recorded C and C_lp (the CPU test
tests/test_sampling_topk_ref.py shows that the general cases pin the kept set and where the constants come from),
bit-equality with nm_gumbel_argmax when nothing truncates, reproducibility, the salt word, the all_finished flag, the
degenerate rows, and the distribution of the draws under top-k."""
import numpy as np
import pytest
import torch

from . import sampling_cases as SC
from . import sampling_ref as SR

pytestmark = pytest.mark.gpu


def _word(value, dev):
    return torch.as_tensor(np.array([value & 0xFFFFFFFF], np.uint32).view(np.int32)).to(dev)


def _step(dev, x, inv_t, top_k, top_p, salt, fin, lps, lens, allfin=None, end=SC.END, step=77):
    """One call; ``x`` is a device view [rows, V]; the salt is split into the device word and the launch argument."""
    from neuralmonkey_amd import ops
    rows = x.shape[0]
    i32 = lambda: torch.full((rows,), -7, dtype=torch.int32, device=dev)
    f32 = lambda: torch.full((rows,), -7.0, dtype=torch.float32, device=dev)
    out = dict(symbol=i32(), logprob=f32(), kept=i32(), finished=i32(), logprob_sum=f32(), lengths=i32())
    ops.sample_step(x, _word(salt - step, dev), step, end, torch.tensor(np.asarray(fin, np.int32)).to(dev),
                    torch.tensor(np.asarray(lps, np.float32)).to(dev),
                    torch.tensor(np.asarray(lens, np.int32)).to(dev), out["symbol"], out["logprob"], out["kept"],
                    out["finished"], out["logprob_sum"], out["lengths"], top_k=top_k, top_p=top_p,
                    inv_temperature=float(np.float32(inv_t)), all_finished=allfin)
    return SR.StepOut(**{k: v.cpu().numpy() for k, v in out.items()})


def _case(dev, b, **kw):
    c = b.case
    x = torch.tensor(b.x).to(dev)[:, :c.v]
    return _step(dev, x, c.inv_t, c.top_k, c.top_p, kw.pop("salt", c.salt), b.finished, b.lps, b.lens, **kw)


@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_every_case_meets_the_rule(dev, name):
    b = SC.build(name)
    got = _case(dev, b)
    errors, hits, live = SR.check_step(b.ref, got, SC.C, SC.C_LP, b.exact)
    print(name, "exact draws", hits, "of", live)
    assert errors == []
    assert hits >= live - int(0.05 * live)
    again = _case(dev, b)                                # two runs are bit-equal in every output
    for first, second in zip(got, again):
        assert np.array_equal(first.view(np.int32), second.view(np.int32))


@pytest.mark.parametrize("rows,vocab,pad", [(3, 7, 0), (37, 1001, 3), (16, 32000, 0), (4, SC.LDS_MAX + 1, 0)])
def test_untruncated_draw_is_bit_equal_to_gumbel_argmax(dev, rows, vocab, pad):
    from neuralmonkey_amd import ops
    g = torch.Generator(device=dev).manual_seed(rows)
    x = (torch.randn(rows, vocab + pad, device=dev, generator=g) * 2.0)[:, :vocab]
    want = torch.empty(rows, dtype=torch.int32, device=dev)
    zeros = np.zeros(rows, np.int32)
    for salt in (0, 12345, 0xFFFFFFFF):
        ops.gumbel_argmax(x, salt, want)
        for top_k in (0, vocab, vocab + 5):
            got = _step(dev, x, 1.0, top_k, 1.0, salt, zeros, np.zeros(rows, np.float32), zeros)
            assert np.array_equal(got.symbol, want.cpu().numpy())
            assert (got.kept == vocab).all()


def test_another_salt_base_draws_differently_and_the_step_adds_to_it(dev):
    b = SC.build("g_v1001_k40_p05")
    one = _case(dev, b, salt=1000)
    two = _case(dev, b, salt=1001)
    assert np.array_equal(one.kept, two.kept) and not np.array_equal(one.symbol, two.symbol)
    assert np.array_equal(one.symbol, _case(dev, b, salt=1000, step=5).symbol)      # base 995 + step 5


def test_all_finished_flag_with_both_presets(dev):
    rows, vocab = 6, 50
    x = torch.zeros(rows, vocab, device=dev)
    x[:, 9] = 40.0                                       # every live row draws column 9
    zeros, lps = np.zeros(rows, np.int32), np.zeros(rows, np.float32)
    fin = np.array([0, 1, 0, 1, 1, 0], np.int32)
    for preset, end, want in ((1, 9, 1), (0, 9, 0), (1, 3, 0), (0, 3, 0)):
        flag = torch.full((1,), preset, dtype=torch.int32, device=dev)
        got = _step(dev, x, 1.0, 5, 0.9, 4, fin, lps, zeros, allfin=flag, end=end)
        assert (got.symbol == np.where(fin, 0, 9)).all()
        assert int(flag.item()) == want
        assert (got.finished == (1 if end == 9 else fin)).all()
    flag = torch.ones(1, dtype=torch.int32, device=dev)   # every row finished before the step: the flag stays
    _step(dev, x, 1.0, 5, 0.9, 4, np.ones(rows, np.int32), lps, zeros, allfin=flag)
    assert int(flag.item()) == 1


@pytest.mark.parametrize("top_k,top_p", [(0, 1.0), (3, 1.0), (0, 0.5), (3, 0.5)])
def test_degenerate_rows_still_yield_a_symbol(dev, top_k, top_p):
    vocab = 300
    x = torch.randn(5, vocab, device=dev)
    x[0] = float("nan")
    x[1] = float("-inf")
    x[2, ::2] = float("nan")
    x[3, 5] = float("inf")
    zeros = np.zeros(5, np.int32)
    got = _step(dev, x, 1.0, top_k, top_p, 11, zeros, np.zeros(5, np.float32), zeros)
    assert ((got.symbol >= 0) & (got.symbol < vocab)).all()
    assert got.symbol[3] == 5 and got.symbol[2] % 2 == 1
    assert (got.lengths == 1).all()


def test_draws_follow_the_renormalised_top_k_distribution(dev):
    logits = np.log(np.array([0.5, 0.25, 0.125, 0.0625, 0.0625], np.float32))
    rows = 1 << 16
    x = torch.as_tensor(np.tile(logits, (rows, 1))).to(dev)
    zeros = np.zeros(rows, np.int32)
    got = _step(dev, x, 1.0, 3, 1.0, 99, zeros, np.zeros(rows, np.float32), zeros)
    counts = np.bincount(got.symbol, minlength=5)
    p = np.array([4, 2, 1, 0, 0]) / 7.0
    sigma = np.sqrt(rows * p * (1 - p))
    assert counts[3] == counts[4] == 0
    assert (np.abs(counts - rows * p)[:3] < 5 * sigma[:3]).all(), counts
    assert (got.kept == 3).all()
    assert np.allclose(got.logprob, np.log(p[got.symbol]), atol=1e-6)
