"""One large GEMM shape, repeated -- the target of PMC passes (MFMA busy cycles, wait buckets) and of a quick timing:
    rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES ... -- python tools/gemm_one.py NN
    python tools/gemm_one.py TN ring --time          microseconds per launch, LDS-ring loop (gemm_ring)
    python tools/gemm_one.py TN tiled --time         the same product through gemm_tiled's loop
    python tools/gemm_one.py TN ring --time --bg     residency-capped background launch (nm_gemm_f32 algo 4)
The loop: ``ring`` / ``tiled`` set NM_GEMM_CFG=10 / 1 before the library's context reads it; without the argument
the library's default runs."""
import os
import sys

LOOPS = {"ring": "10", "tiled": "1"}
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if len(args) > 1:
    os.environ["NM_GEMM_CFG"] = LOOPS[args[1]]

import torch  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from neuralmonkey_amd import ops  # noqa: E402

SHAPES = {"NN": (6400, 32000, 512, False, False), "NT": (6400, 512, 32000, False, True),
          "TN": (512, 32000, 6400, True, False)}


def main():
    kind = args[0] if args else "NN"
    m, n, k, ta, tb = SHAPES[kind]
    algo = ops.GEMM_BACKGROUND if "--bg" in sys.argv else 0
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)
    a = rn(k, m) if ta else rn(m, k)
    b = rn(n, k) if tb else rn(k, n)
    c = torch.empty(m, n, device=dev)
    for _ in range(12):
        ops.gemm(a, b, out=c, trans_a=ta, trans_b=tb, algo=algo)
    torch.cuda.synchronize()
    if "--time" in sys.argv:
        reps = 50
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            ops.gemm(a, b, out=c, trans_a=ta, trans_b=tb, algo=algo)
        end.record()
        torch.cuda.synchronize()
        us = start.elapsed_time(end) * 1e3 / reps
        print("{} {} {}: {:.1f} us per launch, {:.1f} TFLOP/s".format(
            kind, args[1] if len(args) > 1 else "default", "background" if algo else "foreground", us,
            2.0 * m * n * k / us / 1e6))


if __name__ == "__main__":
    main()
