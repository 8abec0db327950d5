"""The case table of the decoder-step sweep (tests/step_group_cases.py) against the library's own dispatch rule,
without a GPU: nm_step_group_plan names the kernel nm_step_group would launch and launches nothing, so what each case
was written for is checked here, on every machine -- a tuning change that moves a case to another kernel fails this
module instead of silently thinning the GPU sweep.  (step_group_dma_kernel needs a device to be chosen: its cases are
checked by the GPU module.)"""
import ctypes

import pytest

from . import step_group_cases as SC


@pytest.fixture
def default_switches(monkeypatch):
    """A context that read the default switches, bound to this thread (the process default context may have been
    created under another environment)."""
    from neuralmonkey_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    for name in ("NM_STEP_MEDIUM", "NM_STEP_DMA"):
        monkeypatch.delenv(name, raising=False)
    ctx = ctypes.c_void_p()
    assert lib.nm_create(0, ctypes.byref(ctx)) == 0
    assert lib.nm_ctx_bind(ctx) == 0
    yield lib
    assert lib.nm_ctx_bind(None) == 0 and lib.nm_destroy(ctx) == 0


def plan_of(case):
    from neuralmonkey_amd import ops
    return ops.StepGroup(case.m, SC.placeholder_specs(case)).plan()


def test_every_case_reaches_the_instance_it_was_written_for(default_switches):
    for case in SC.CASES:
        assert plan_of(case) == case.want, case.name
    for name, m, n, k, want, dma in SC.PERMUTATIONS:
        if not dma:
            assert plan_of(SC.C(name, m, [SC.P(n, k, bias=False)], want)) == want, name


def test_table_reaches_every_instance_and_both_sides_of_every_boundary(default_switches):
    from neuralmonkey_amd import ops
    plans = {case.name: plan_of(case) for case in SC.CASES}
    counts = {case.name: SC.tile_counts(case) for case in SC.CASES}
    # every a_kind-0 instance that needs no device to be chosen (the a_kind-1 one and the DMA one: GPU module)
    assert set(plans.values()) == set(ops.STEP_GROUP_PLANS) - {"16x1-partials", "dma"}
    assert {case.want_dma for case in SC.CASES} >= {"dma"}

    def sides(below, above):
        lo = {plans[c.name] for c in SC.CASES if below(c, *counts[c.name])}
        hi = {plans[c.name] for c in SC.CASES if above(c, *counts[c.name])}
        return lo, hi

    medium = {"medium-4x2x2", "medium-8x1x1", "medium-4x1x1"}
    # M = 256 / 257
    lo, hi = sides(lambda c, *_: c.m == 256, lambda c, *_: c.m == 257)
    assert lo and hi and lo <= {"16x1", "16x2"} and hi <= medium
    # 512 / 513 tiles of 16x16
    lo, hi = sides(lambda c, t16, *_: c.m <= 256 and t16 == 512, lambda c, t16, *_: c.m <= 256 and t16 == 513)
    assert lo == {"16x1"} and hi == {"16x2"}
    # 255 / 256 tiles of 64x64
    lo, hi = sides(lambda c, _, t64, __: c.m > 256 and t64 == 255, lambda c, _, t64, __: c.m > 256 and t64 == 256)
    assert lo and hi == {"medium-4x2x2"} and not lo & hi
    # grid 640 / the next reachable one (641 is prime and a grid has at least nine tile rows): 650
    lo, hi = sides(lambda c, _, t64, t32: c.m > 256 and t64 < 256 and t32 == 640,
                   lambda c, _, t64, t32: c.m > 256 and t64 < 256 and 640 < t32 <= 650)
    assert lo == {"medium-8x1x1"} and hi == {"medium-4x1x1"}


def test_plan_refuses_what_the_launch_refuses(default_switches):
    from neuralmonkey_amd import _lib, ops
    ok = SC.placeholder_specs(SC.CASES[0])
    assert ops.StepGroup(260, ok).plan() == "medium-4x2x2"
    for field, value, text in (("K", 40, "multiple of 16"), ("epilogue", 3, "bad epilogue"), ("lda", 46, "A must be"),
                               ("a_kind", 1, "attention partials"), ("act", 2, "bad plain epilogue")):
        bad = [dict(s) for s in ok]
        bad[1][field] = value
        with pytest.raises(_lib.NMHipError, match=text):
            ops.StepGroup(260, bad).plan()
    with pytest.raises(_lib.NMHipError, match="bad M"):
        ops.StepGroup(0, ok).plan()
    # nine attention partials (source length 97) are one more than the operand loader holds
    addr = 0x10000
    part = dict(a_kind=1, Bt=addr, ldb=48, N=20, K=48, epilogue=0, act=1, C=addr, ldc=20, pctx=addr, pstat=addr, nchunk=8)
    assert ops.StepGroup(5, [part]).plan() == "16x1-partials"
    with pytest.raises(_lib.NMHipError, match="1..8 chunks"):
        ops.StepGroup(5, [dict(part, nchunk=9)]).plan()
