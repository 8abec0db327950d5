"""HIP-event timings of the frozen VGG-16 stack of encoders/imagenet_encoder.py: every distinct 3 x 3 layer shape of VGG-16
(nine shapes cover its 13 convolutions) at B = 5 (tests/captioning.ini's batch) and B = 32, the fused kernel
nm_conv2d_act_fwd under each of its tiles and under its automatic choice against what the commit before it would run --
nm_conv2d_fwd followed by a ReLU pass -- and the whole stack to conv5_3 (13 convolutions, 4 poolings) on both routes.
The variants of a shape are timed in interleaved rounds in one process; a figure is the median over the rounds of
``--reps`` calls between two events.  Prints one JSON line: per batch and shape the times, TFLOP/s and the fraction of the
157.3 TFLOP/s fp32 matrix peak, the faster route, and the whole-stack times.

    timeout -k 10 500 python tools/bench_vgg.py [--rounds 7] [--out profiles/vgg_bench.json]

Every measured shape also has a time limit of its own (``--step-timeout`` seconds, checked between calls): a shape that
overruns it ends the run with exit status 3 instead of starting the next one.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmonkey_amd import ops                                         # noqa: E402
from neuralmonkey_amd.encoders import imagenet_encoder as net            # noqa: E402

PEAK_TFLOPS = 157.3
TILES = ["auto", "128x64", "64x64"]
LAST = "vgg_16/conv5/conv5_3"


class StepTimeout(RuntimeError):
    pass


def distinct_shapes():
    """[(name, (H, W, Cin, Cout), [the layers of that shape])] of VGG-16's convolutions, in order."""
    found = {}
    for layer in net.layer_table("vgg_16"):
        if layer.kind == "conv":
            found.setdefault(layer.in_hw + (layer.cin, layer.cout), []).append(layer.endpoint.rsplit("/", 1)[1])
    return [("{}x{}_{}to{}".format(*shape), shape, names) for shape, names in found.items()]


def interleaved(variants, rounds, reps, limit):
    """name -> median milliseconds of one call; ``variants``: name -> callable."""
    t0 = time.monotonic()
    for fn in variants.values():
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            if time.monotonic() - t0 > limit:
                raise StepTimeout("a measured shape ran past {} s".format(limit))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / reps)
    return {name: sorted(vals)[len(vals) // 2] for name, vals in times.items()}


def rate(ms, flop):
    return {"ms": round(ms, 4), "tflops": round(flop / ms / 1e9, 2), "of_peak": round(flop / ms / 1e9 / PEAK_TFLOPS, 4)}


def measure_shape(dev, bsz, shape, rounds, reps, limit):
    h, w, cin, cout = shape
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(bsz, h, w, cin, device=dev, generator=g)
    filt = torch.randn(3, 3, cin, cout, device=dev, generator=g) / (9 * cin) ** 0.5
    bias = torch.randn(cout, device=dev, generator=g) * 0.1
    y = torch.empty(bsz, h, w, cout, device=dev)
    flat = y.view(-1, cout)

    def parent():
        ops.conv2d_fwd(x, filt, bias, y, "same")
        ops.ew("relu", flat, None, flat)
    variants = {"conv2d+relu": parent}
    for tile in TILES:
        variants["act_" + tile] = lambda tile=tile: ops.conv2d_act_fwd(x, filt, bias, y, "same", relu=True, tile=tile)
    ms = interleaved(variants, rounds, reps, limit)
    flop = 2.0 * bsz * h * w * 9 * cin * cout
    res = {name: rate(val, flop) for name, val in ms.items()}
    res["gflop"] = round(flop / 1e9, 3)
    res["faster"] = "act" if ms["act_auto"] <= ms["conv2d+relu"] else "conv2d+relu"
    res["speedup"] = round(ms["conv2d+relu"] / ms["act_auto"], 3)
    return res


def measure_stack(dev, bsz, rounds, limit):
    plan = []
    for layer in net.layer_table("vgg_16"):
        plan.append(layer)
        if layer.endpoint == LAST:
            break
    g = torch.Generator(device=dev).manual_seed(2)
    images = torch.randn(bsz, 224, 224, 3, device=dev, generator=g) * 60.0
    variables, buffers, flop = {}, {}, 0.0
    for layer in plan:
        buffers[layer.endpoint] = torch.empty((bsz,) + layer.out_hw + (layer.cout,), device=dev)
        for name, shape in layer.variables:
            scale = (9 * layer.cin) ** -0.5 if name.endswith("weights") else 0.1
            variables[name] = torch.randn(shape, device=dev, generator=g) * scale
        if layer.kind == "conv":
            flop += 2.0 * bsz * layer.out_hw[0] * layer.out_hw[1] * 9 * layer.cin * layer.cout

    def run(route):
        net.run_layers(plan, images, variables.__getitem__, lambda endpoint, shape: buffers[endpoint], route=route)
    ms = interleaved({"dispatch": lambda: run(net.conv_route), "act": lambda: run(lambda b, l: "act"),
                      "conv2d+relu": lambda: run(lambda b, l: "conv2d+relu")}, rounds, 1, limit)
    res = {name: rate(val, flop) for name, val in ms.items()}
    res["gflop"] = round(flop / 1e9, 2)
    res["speedup"] = round(ms["conv2d+relu"] / ms["dispatch"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[5, 32])
    ap.add_argument("--step-timeout", type=float, default=60.0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"peak_tflops": PEAK_TFLOPS, "device": torch.cuda.get_device_name(0)}
    code = 0
    try:
        for bsz in args.batches:
            per = out.setdefault("B{}".format(bsz), {"layers": {}})
            for name, shape, layers in distinct_shapes():
                per["layers"][name] = dict(measure_shape(dev, bsz, shape, args.rounds, args.reps, args.step_timeout),
                                           covers=layers)
            per["stack_to_conv5_3"] = measure_stack(dev, bsz, args.rounds, args.step_timeout)
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
