"""HIP-event timings of one residual layer of the convolutional sequence-to-sequence encoder (nm_conv1d_glu_fwd /
nm_conv1d_glu_bwd) at the roofline shape of DESIGN.md section 4.12 (B*T = 4096, C = 512, w = 5) and at the shape of
the reference's tests/bpe.ini (B = 16, T = 10, C = 10, w = 5).  Warm-up, then the median of ``--iters`` event-timed
calls.  Prints one JSON line: per shape the forward (auto and forced scalar) and the backward time, TFLOP/s and the
fraction of the 157.3 TFLOP/s fp32 MFMA peak.

    timeout -k 10 120 python tools/convs2s_bench.py [--iters 20]

Every measured step also has a time limit of its own (``--step-timeout`` seconds, checked between calls): a step that
overruns it ends the run with exit status 3 instead of starting the next one.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmonkey_amd import ops             # noqa: E402

PEAK_TFLOPS = 157.3
SHAPES = {"roofline": (16, 256, 512, 5), "bpe_ini": (16, 10, 10, 5)}


class StepTimeout(RuntimeError):
    pass


def timed(fn, iters, limit):
    t0 = time.monotonic()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        if time.monotonic() - t0 > limit:
            raise StepTimeout("a measured step ran past {} s".format(limit))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def measure(dev, shape, iters, limit):
    bsz, steps, c, width = shape
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(bsz, steps, c, device=dev, generator=g)
    w = torch.randn(width, c, 2 * c, device=dev, generator=g) * (4.0 / c / width) ** 0.5
    b = torch.randn(2 * c, device=dev, generator=g) * 0.1
    dy = torch.randn(bsz, steps, c, device=dev, generator=g)
    y = torch.empty_like(x)
    lin, sig = torch.empty(bsz * steps, c, device=dev), torch.empty(bsz * steps, c, device=dev)
    dz = torch.empty(bsz * steps, 2 * c, device=dev)
    dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
    wsp = torch.empty(max(1, ops.conv1d_glu_workspace_floats(bsz, steps, c, width)), device=dev)
    flop = 2.0 * bsz * steps * width * c * 2 * c
    res = {"shape": {"B": bsz, "T": steps, "C": c, "w": width}, "gflop": round(flop / 1e9, 3),
           "mfma_floor_ms": round(flop / PEAK_TFLOPS / 1e9, 4)}

    def put(name, ms, f):
        res[name] = {"ms": round(ms, 4), "tflops": round(f / ms / 1e9, 3), "of_peak": round(f / ms / 1e9 / PEAK_TFLOPS, 4)}
    put("fwd", timed(lambda: ops.conv1d_glu_fwd(x, w, b, y, lin, sig), iters, limit), flop)
    put("fwd_inference", timed(lambda: ops.conv1d_glu_fwd(x, w, b, y), iters, limit), flop)
    put("fwd_scalar", timed(lambda: ops.conv1d_glu_fwd(x, w, b, y, lin, sig, algo=2), max(3, iters // 4), limit), flop)
    put("bwd", timed(lambda: ops.conv1d_glu_bwd(x, w, lin, sig, dy, dz, dx=dx, dfilt=dw, dbias=db,
                                                accumulate_params=False, workspace=wsp), iters, limit), 2 * flop)
    put("bwd_dx_only", timed(lambda: ops.conv1d_glu_bwd(x, w, lin, sig, dy, dz, dx=dx), iters, limit), flop)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-timeout", type=float, default=30.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    try:
        for name, shape in SHAPES.items():
            out[name] = measure(dev, shape, args.iters, args.step_timeout)
    except StepTimeout as exc:
        print(json.dumps({"error": str(exc), "partial": out}))
        sys.exit(3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
