"""HIP-event timings of the image stack's convolution (nm_conv2d_fwd / nm_conv2d_bwd), both algorithms, at a realistic
scene-text shape (B = 64, 32 x 256, 3 x 3 SAME, 64 -> 128 channels) and at the first and the widest convolution of the
reference's tests/str.ini (B = 4: 32 x 256 x 1 -> 4 VALID, and 15 x 127 x 12 -> 12 SAME).  Warm-up, then the median of
``--iters`` event-timed calls.  Prints one JSON line: per shape and algorithm the forward and the backward time, TFLOP/s
and the fraction of the 157.3 TFLOP/s fp32 MFMA peak.

    timeout -k 10 300 python tools/bench_conv2d.py [--iters 10] [--out profiles/conv2d_bench.json]

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
# name -> (B, H, W, Cin, Cout, k, padding)
SHAPES = {"scene_text": (64, 32, 256, 64, 128, 3, "same"), "str_ini_first": (4, 32, 256, 1, 4, 3, "valid"),
          "str_ini_widest": (4, 15, 127, 12, 12, 3, "same")}
ALGOS = {"mfma": 1, "scalar": 2, "auto": 0}


class StepTimeout(RuntimeError):
    pass


def timed(fn, iters, limit):
    t0 = time.monotonic()
    for _ in range(2):
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
    bsz, h, w, cin, cout, k, pad = shape
    g = torch.Generator(device=dev).manual_seed(1)
    oh, ow = ops.conv2d_out_hw(h, w, k, pad)
    x = torch.randn(bsz, h, w, cin, device=dev, generator=g)
    filt = torch.randn(k, k, cin, cout, device=dev, generator=g) / (k * k * cin) ** 0.5
    bias = torch.randn(cout, device=dev, generator=g) * 0.1
    dy = torch.randn(bsz, oh, ow, cout, device=dev, generator=g)
    y = torch.empty(bsz, oh, ow, cout, device=dev)
    dx, dw, db = torch.empty_like(x), torch.empty_like(filt), torch.empty_like(bias)
    wsp = torch.empty(max(1, ops.conv2d_workspace_floats(bsz, h, w, cin, k, cout, pad)), device=dev)
    flop = 2.0 * bsz * oh * ow * k * k * cin * cout
    res = {"shape": {"B": bsz, "H": h, "W": w, "Cin": cin, "Cout": cout, "k": k, "padding": pad},
           "gflop": round(flop / 1e9, 4), "mfma_floor_ms": round(flop / PEAK_TFLOPS / 1e9, 5)}

    def put(name, ms, f):
        res[name] = {"ms": round(ms, 4), "tflops": round(f / ms / 1e9, 3), "of_peak": round(f / ms / 1e9 / PEAK_TFLOPS, 4)}
    for tag, algo in ALGOS.items():
        n = iters if tag != "scalar" else max(3, iters // 3)
        put("fwd_" + tag, timed(lambda: ops.conv2d_fwd(x, filt, bias, y, pad, algo=algo), n, limit), flop)
        put("bwd_" + tag, timed(lambda: ops.conv2d_bwd(x, filt, dy, pad, dx=dx, dfilt=dw, dbias=db, accumulate_params=False,
                                                       workspace=wsp, algo=algo), n, limit), 2 * flop)
        put("bwd_dx_only_" + tag, timed(lambda: ops.conv2d_bwd(x, filt, dy, pad, dx=dx, algo=algo), n, limit), flop)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-timeout", type=float, default=60.0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    code = 0
    try:
        for name, shape in SHAPES.items():
            out[name] = measure(dev, shape, args.iters, args.step_timeout)
    except StepTimeout as exc:
        out = {"error": str(exc), "partial": out}
        code = 3
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as handle:
            handle.write(line + "\n")
    sys.exit(code)


if __name__ == "__main__":
    main()
