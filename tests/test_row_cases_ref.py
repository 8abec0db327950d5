"""tests/row_cases.py on the CPU: what the GPU tests of the vocabulary-row kernels (tests/test_row_kernels_gpu.py) rely
on.

1. Coverage: the table reaches every branch of the three restated dispatch rules, with a case on each side of every
   boundary, and holds the sizes, layouts, targets and options it is meant to hold.
2. Tolerances: the float32 numpy restatement of each operation stays within the recorded E_* of the float64 reference
   over the whole table, the E_* have not drifted, every C_* is at most about ten times its E_* and none is looser
   than the ceilings of tests/test_kernels_gpu.py (1e-6 for the lse, 1e-5 for loss and gradient) -- but for the
   smoothed loss of logits near +-1e4, where the restatement itself exceeds the ceiling and which is kept apart.
3. Ties and degenerate rows pin one answer.
4. The draws: for the table's seeds the float32 restated draw equals the float64 one in every row under every salt and
   wins by more than the 1e-4 of the rule, so the 95 % of the GPU test are reachable and the rule pins the symbol."""
import numpy as np
import pytest

from oracle.nm_oracle import gumbel_noise

from . import row_cases as RC


# ------------------------------------------------------------------------------------------------------------------
# 1. coverage
# ------------------------------------------------------------------------------------------------------------------
def _rule(fn, cases):
    return {fn(lay.v, lay.ldx, lay.aligned) for lay in (RC.layout(c.v, c.variant) for c in cases)}


def test_row_statistics_table_reaches_every_branch_and_both_sides_of_every_boundary():
    assert _rule(RC.row_scan_nv, RC.STATS_CASES) == set(RC.SCAN_BRANCHES)
    assert {c.v for c in RC.STATS_CASES} == set(RC.STATS_V)
    for below, branch_below, branch_above in ((8192, "scan8", "scan16"), (16384, "scan16", "scan32"),
                                              (32768, "scan32", "scalar:V>131072")):
        for variant in ("plain", "ld4"):                 # float4s per row: 8192 | 8193, 16384 | 16385, 32768 | 32769
            lo, hi = RC.layout(4 * below, variant), RC.layout(4 * below + 4, variant)
            assert RC.row_scan_nv(lo.v, lo.ldx, lo.aligned) == branch_below
            assert RC.row_scan_nv(hi.v, hi.ldx, hi.aligned) == branch_above
            assert {"s_v{}_{}_values".format(lo.v, variant), "s_v{}_{}_ties".format(hi.v, variant)} <= set(RC.STATS_BY_NAME)
    for v in RC.STATS_V:
        if v % 4 == 0:
            assert {c.variant for c in RC.STATS_CASES if c.v == v} == set(RC.VARIANTS)
            for variant in ("ld1", "shift"):             # the scalar kernel by rule
                lay = RC.layout(v, variant)
                assert RC.row_scan_nv(lay.v, lay.ldx, lay.aligned).startswith("scalar:")
            lay = RC.layout(v, "ld4")
            assert lay.ldx == v + 4 and (v > 131072 or RC.row_scan_nv(lay.v, lay.ldx, True).startswith("scan"))
    kinds = {k for c in RC.STATS_CASES for k in RC.stats_kinds(c.v, c.group)}
    assert kinds == {"normal", "plus1e4", "minus1e4", "all_equal", "quarter_ninf", "one_finite", "max_last",
                     "max_lane0", "max_lane1", "max_lane2", "max_lane3", "tie_thread", "tie_lanes", "tie_waves",
                     "tie_first_last"}
    assert all(1 <= len(RC.stats_kinds(c.v, c.group)) <= 7 for c in RC.STATS_CASES)
    for name in RC.SUBSET_CASES:
        assert name in RC.STATS_BY_NAME
    vec, sca = (RC.layout(RC.STATS_BY_NAME[n].v, RC.STATS_BY_NAME[n].variant) for n in RC.SUBSET_CASES)
    assert RC.row_scan_nv(*vec[:2], vec.aligned) == "scan8" and RC.row_scan_nv(*sca[:2], sca.aligned) == "scalar:ldx%4"
    assert [RC.row_scan_nv(v, v, True)[:4] for v, _ in RC.DEGENERATE_LAYOUTS] == ["scan", "scal"]


def test_cross_entropy_table_reaches_every_branch_and_both_sides_of_every_boundary():
    assert _rule(RC.xent_nv, RC.XENT_CASES) == set(RC.XENT_BRANCHES)
    assert {c.v for c in RC.XENT_CASES} == set(RC.XENT_V)
    assert RC.xent_nv(32768, 32768, True) == "regs8" and RC.xent_nv(32772, 32772, True) == "regs16"      # 8192 float4s
    assert RC.xent_nv(65536, 65536, True) == "regs16" and RC.xent_nv(65540, 65540, True) == "scalar:V>65536"
    for v in RC.XENT_V:
        here = [c for c in RC.XENT_CASES if c.v == v]
        assert {c.variant for c in here} == (set(RC.VARIANTS) if v % 4 == 0 else {"plain"})
        for variant in {c.variant for c in here}:
            assert {(c.eps, c.targets) for c in here if c.variant == variant} >= \
                {(0.0, "in"), (0.0, "edge"), (0.1, "in"), (0.1, "edge")}
    # targets: the ends, each float4 lane, 4095 / 4096 / 4097, and the three kinds outside [0, V)
    tin, tedge = RC.xent_targets(65536, "in"), RC.xent_targets(65536, "edge")
    assert {0, 65535} <= set(tin) and {t % 4 for t in tin} == {0, 1, 2, 3}
    assert tedge == [4095, 4096, 4097, -1, 65536, RC.INT_MAX]
    assert all(1 <= len(RC.xent_targets(c.v, c.targets)) <= 7 for c in RC.XENT_CASES)
    # every combination of the three optional arguments at two sizes, one per kind of kernel
    for v, variant in RC.XENT_OPTION_LAYOUTS:
        assert len({c.options for c in RC.XENT_CASES if (c.v, c.variant) == (v, variant)}) == 8
    assert {RC.xent_nv(v, v, True)[:4] for v, _ in RC.XENT_OPTION_LAYOUTS} == {"regs", "scal"}
    # the contents, on both register kernels and the scalar one
    for content in ("plus1e4", "minus1e4", "ninf"):
        hit = _rule(RC.xent_nv, [c for c in RC.XENT_CASES if c.content == content])
        assert {"regs8", "regs16"} <= hit and any(b.startswith("scalar") for b in hit)
    assert all(c.eps == 0 for c in RC.XENT_CASES if c.content == "ninf")
    b = RC.build_xent("x_v4096_plain_eps0_in_ninf")
    assert (np.isinf(b.x).mean(1) > 0.2).all() and np.isfinite(b.x[np.arange(b.rows), b.targets]).all()
    assert np.isinf(b.x[:, :4]).any(1).all()             # a masked class among thread 0's columns
    b = RC.build_xent("x_v4100_plain_eps01_in_normal")
    assert (b.weights == 0).sum() == 1 and (b.weights < 0).sum() == 1


def test_column_sum_table_reaches_every_branch_and_both_sides_of_every_boundary():
    hit = set()
    for c in RC.COLS_CASES:
        lay = RC.layout(c.v, c.variant)
        hit.add(RC.colsum_nv(lay.v, lay.ldx, lay.aligned, True, c.rows, c.g))
    for what, v, extra, off, poff, rows, g in RC.COLS_REFUSALS:
        branch = RC.colsum_nv(v, v + extra, off % 4 == 0, poff % 4 == 0, rows, g)
        assert branch.startswith("refuse:"), what
        hit.add(branch)
    assert hit == set(RC.COLS_BRANCHES)
    # 2048 | 4096 | 8192 float4s: 8192 | 8196 and 16384 | 16388 columns, and the largest size the kernel takes
    assert [RC.colsum_nv(v, v, True, True, 7, 3) for v in (8192, 8196, 16384, 16388, 32768, 32772)] == \
        ["cols2", "cols4", "cols4", "cols8", "cols8", "refuse:V>32768"]
    assert {c.v for c in RC.COLS_CASES} == set(RC.COLS_V)
    for v in RC.COLS_V:
        here = [c for c in RC.COLS_CASES if c.v == v and c.content == "normal"]
        assert {(c.rows, c.g, c.variant, c.eps) for c in here} == \
            {(r, g, va, e) for r, g in RC.COLS_ROWS_G for va in ("plain", "ld4") for e in (0.0, 0.1)}
    outside = sum(int(((b.targets < 0) | (b.targets >= b.case.v)).sum())
                  for b in (RC.build_cols(c.name) for c in RC.COLS_CASES if c.v <= 1024))
    assert outside > 20
    assert {w for w, *_ in RC.COLS_REFUSALS} >= {"V%4", "V=32772", "G=0", "G>rows", "partial off alignment"}


def test_draw_table():
    assert {(c.rows, c.v, c.pad) for c in RC.DRAW_CASES} == {(1, 1, 0), (5, 1, 3), (7, 255, 0), (7, 256, 4),
                                                             (7, 257, 3), (3, 32001, 1)}
    assert RC.DRAW_SALTS == (0, 12345, 0xFFFFFFFF)


def test_padding_is_3e38_everywhere_outside_the_view():
    for b in (RC.build_stats("s_v64_shift_values"), RC.build_stats("s_v64_ld1_ties"), RC.build_xent("x_v40_ld4_eps0_in_normal")):
        rows = b.x.shape[0]
        mask = RC.padding(rows, b.lay)
        assert mask.sum() == b.flat.size - rows * b.lay.v and (b.flat[mask] == RC.PAD).all()
        assert not (b.flat[~mask] == RC.PAD).any()
    assert RC.build_stats("s_v64_shift_values").flat[0] == RC.PAD       # the float before a shifted view


# ------------------------------------------------------------------------------------------------------------------
# 2. tolerances
# ------------------------------------------------------------------------------------------------------------------
def _within(measured, recorded):
    """the restatement stays within the recorded error, and the record has not drifted from what the table gives"""
    return 0.95 * recorded <= measured <= 1.0005 * recorded


def test_measured_errors_and_the_constants():
    e_lse = 0.0
    for c in RC.STATS_CASES:
        b = RC.build_stats(c.name)
        mx, am, lse = RC.f32_stats(b.x)
        assert np.array_equal(mx, b.max) and np.array_equal(am, b.argmax)
        assert np.isfinite(b.lse).all()
        e_lse = max(e_lse, RC.scaled(lse, b.lse))
    e_loss = e_off = e_g = e_p = e_b = 0.0
    for cases, build in ((RC.XENT_CASES, RC.build_xent), (RC.COLS_CASES, RC.build_cols)):
        for c in cases:
            b = build(c.name)
            assert np.isfinite(b.ref.loss).all() and np.isfinite(b.ref.grad).all(), c.name
            loss, g = RC.f32_xent(b.x, b.targets, b.weights, b.grad_scale, c.eps)
            if b.offset_class:
                e_off = max(e_off, RC.scaled(loss, b.ref.loss))
            else:
                e_loss = max(e_loss, RC.scaled(loss, b.ref.loss))
            e_g = max(e_g, RC.in_units(g, b.ref.grad, b.ref.unit))
            if build is RC.build_cols:
                part, bias = RC.f32_colsum(g, c.g)
                ref_part, unit_part, ref_bias, unit_bias = RC.ref_colsum(b.ref, c.g)
                e_p = max(e_p, RC.in_units(part, ref_part, unit_part))
                e_b = max(e_b, RC.in_units(bias, ref_bias, unit_bias))
    print("float32 restatement over the row table: lse {:.3e}, loss {:.3e}, smoothed loss at +-1e4 {:.3e}, gradient "
          "{:.3e}, partials {:.3e}, bias {:.3e}".format(e_lse, e_loss, e_off, e_g, e_p, e_b))
    assert _within(e_lse, RC.E_LSE), e_lse
    assert _within(e_loss, RC.E_LOSS), e_loss
    assert _within(e_off, RC.E_LOSS_OFFSET), e_off
    assert _within(e_g, RC.E_G), e_g
    assert _within(e_p, RC.E_P), e_p
    assert _within(e_b, RC.E_B), e_b
    assert (RC.E_LSE, RC.E_LOSS, RC.E_LOSS_OFFSET, RC.E_G, RC.E_P, RC.E_B) == \
        (2.321e-7, 1.502e-7, 1.944e-5, 1.223e-6, 1.160e-6, 1.087e-6)
    assert (RC.C_LSE, RC.C_LOSS, RC.C_LOSS_OFFSET, RC.C_G, RC.C_P, RC.C_B) == (1.0e-6, 1.5e-6, 1.9e-4, 1.0e-5, 1.0e-5, 1.0e-5)


def test_bounds_are_at_most_ten_times_the_measured_errors_and_within_the_ceilings():
    for c, e in ((RC.C_LSE, RC.E_LSE), (RC.C_LOSS, RC.E_LOSS), (RC.C_LOSS_OFFSET, RC.E_LOSS_OFFSET), (RC.C_G, RC.E_G),
                 (RC.C_P, RC.E_P), (RC.C_B, RC.E_B)):
        assert 4.0 * e <= c <= 10.05 * e
    assert RC.C_LSE <= 1e-6 and max(RC.C_LOSS, RC.C_G, RC.C_P, RC.C_B) <= 1e-5
    # the class apart: the restatement itself is beyond the ceiling there, and only there
    assert RC.E_LOSS_OFFSET > 1e-5
    apart = [c for c in RC.XENT_CASES if RC.build_xent(c.name).offset_class]
    assert apart and all(c.content in ("plus1e4", "minus1e4") and c.eps > 0 for c in apart)
    assert not any(RC.build_cols(c.name).offset_class for c in RC.COLS_CASES[:4])


def test_the_gradient_unit_sees_a_dropped_smoothing_term_and_a_one_hot_one_lane_off():
    b = RC.build_xent("x_v32768_plain_eps01_in_normal")
    loss, g = RC.f32_xent(b.x, b.targets, b.weights, b.grad_scale, b.case.eps)
    assert RC.in_units(g, b.ref.grad, b.ref.unit) <= RC.E_G
    scale = (b.weights * b.grad_scale)[:, None]
    dropped = g + np.float32(0.1 / 32768) * scale        # `- qu` left out
    assert RC.in_units(dropped, b.ref.grad, b.ref.unit) > 10 * RC.C_G
    moved = g.copy()
    r = int(np.nonzero(b.weights > 0)[0][0])
    t = int(b.targets[r])
    other = t + 1 if t + 1 < b.case.v else t - 1
    moved[r, t] += np.float32(0.9) * scale[r, 0]
    moved[r, other] -= np.float32(0.9) * scale[r, 0]
    assert RC.in_units(moved, b.ref.grad, b.ref.unit) > 1e3


# ------------------------------------------------------------------------------------------------------------------
# 3. ties and degenerate rows: one answer
# ------------------------------------------------------------------------------------------------------------------
def test_tie_rows_pin_the_first_of_their_columns():
    seen = set()
    for c in RC.STATS_CASES:
        b = RC.build_stats(c.name)
        for r, want in b.pinned.items():
            assert b.argmax[r] == want, (c.name, b.kinds[r])
            seen.add(b.kinds[r])
        for r, kind in enumerate(b.kinds):
            if kind.startswith("tie_"):
                hits = np.nonzero(b.x[r] == b.max[r])[0]
                assert len(hits) == 2 and hits[0] == b.pinned[r]
                if kind != "tie_first_last":
                    assert tuple(hits) == {"tie_thread": RC.TIE_THREAD, "tie_lanes": RC.TIE_LANES,
                                           "tie_waves": RC.TIE_WAVES}[kind]
    assert seen >= {"tie_thread", "tie_lanes", "tie_waves", "tie_first_last", "all_equal", "one_finite", "max_last"}
    # the thread / lane / wave a column falls to: float4 q of the vector kernels belongs to thread q % 1024, column c
    # of the scalar ones to thread c % 1024; a wave is 64 threads
    for (a, z), same_thread, same_wave in ((RC.TIE_THREAD, True, True), (RC.TIE_LANES, False, True), (RC.TIE_WAVES, False, False)):
        for ta, tz in (((a // 4) % 1024, (z // 4) % 1024), (a % 1024, z % 1024)):
            assert (ta == tz) == same_thread and (ta // 64 == tz // 64) == same_wave


def test_degenerate_rows_have_one_answer():
    for v, _ in RC.DEGENERATE_LAYOUTS:
        x, want = RC.degenerate_rows(v)
        assert want[1] == 0 == int(np.argmax(x[1]))       # all -inf: the first index, which is np.argmax
        assert want[2] is None and np.isnan(x[2]).all()
        assert want[3] % 2 == 1 and x[3, want[3]] == np.nanmax(x[3]) and np.isnan(x[3, ::2]).all()
        assert want[0] == int(x[0].argmax()) and np.isfinite(x[0]).all()


# ------------------------------------------------------------------------------------------------------------------
# 4. the draws
# ------------------------------------------------------------------------------------------------------------------
def test_restated_uniforms_are_the_oracles():
    for salt in RC.DRAW_SALTS:
        u = RC.gumbel_u(5, 300, salt)
        assert np.array_equal((-np.log(-np.log(u.astype(np.float32)))).astype(np.float32), gumbel_noise(5, 300, salt))


@pytest.mark.parametrize("name", [c.name for c in RC.DRAW_CASES])
def test_float32_restated_draw_alone_meets_the_95_percent_and_the_rule_pins_it(name):
    c = RC.DRAW_BY_NAME[name]
    lay, flat, x = RC.build_draw(name)
    assert (flat[RC.padding(c.rows, lay)] == RC.PAD).all()
    for salt in RC.DRAW_SALTS:
        got, noisy = RC.f32_draw(x, salt)
        assert (got == RC.ref_draw(x, salt)).mean() >= 0.95
        assert (got == RC.ref_draw(x, salt)).all()        # at 1 to 7 rows 95 % is every row
        if c.v > 1:
            ranked = np.sort(noisy, 1)
            assert ((ranked[:, -1] - ranked[:, -2]) > 10 * RC.DRAW_GAP).all()
        else:
            assert (got == 0).all()
