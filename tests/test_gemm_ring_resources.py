"""Registers, LDS and scratch of the LDS-ring GEMM kernel (gemm_ring, neuralmonkey_amd/csrc/nm_gemm.hip), read from
the built library's code objects (tools/kernel_resources.py; no GPU).  The ring keeps three k-tiles in LDS so that a
workgroup does not need neighbours to keep the matrix pipe busy -- but it must not cost the neighbours either: three
stages are 50 688 B (three workgroups in a CU's 160 KB), and the registers have to leave at least two workgroups of
8 waves per CU.  Residency-capped background launches (nm_gemm_f32 algo 4) take the ring as well, beside a cluster time
loop that is budgeted against a GEMM of at most 80 vector registers and 64 KB of its own LDS
(tests/test_abi.py::test_register_budgets_of_the_overlapped_kernels), so every instance has to stay within those."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ring_kernels():
    from neuralmonkey_amd import _lib
    _lib.load()                                     # the library is built
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_resources
    finally:
        sys.path.pop(0)
    table = kernel_resources()
    return table, {k: v for k, v in table.items() if re.match(r"_Z9gemm_ringILb[01]ELb[01]ELb[01]EE", k)}


def test_every_instance_fits_three_to_a_cu_without_scratch():
    _, ring = ring_kernels()
    assert len(ring) == 8                           # transA x transB x vector / scalar loads
    for name, v in ring.items():
        assert v["max_threads"] == 512 and v["scratch"] == 0, name
        assert v["lds"] <= 50688, (name, v["lds"])
        waves_per_simd = 512 // v["arch_vgprs"]     # 8 waves per workgroup = 2 per SIMD
        assert waves_per_simd // 2 >= 2, (name, v["arch_vgprs"])


def test_background_launches_keep_the_budget_of_the_loop_they_replace():
    table, ring = ring_kernels()
    loops = [v["arch_vgprs"] for k, v in table.items() if "gru_cluster_" in k or "nematus_cluster_" in k]
    assert len(loops) == 8
    for name, v in ring.items():
        assert v["arch_vgprs"] <= 80 and v["lds"] <= 64 * 1024, (name, v)
        assert 2 * max(loops) + 2 * v["arch_vgprs"] <= 512, name
