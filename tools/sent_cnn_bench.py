"""HIP-event timings of the sentence CNN encoder's kernels at the paper's sizes (Lee, Cho & Hofmann 2017) and the
engine's batch: B = 128, S = 250 characters, E = 128, widths 1-8 with 200/200/250/250/300/300/300/300 filters, segments
of 5 (50 pooled positions), four highway layers of 2100.  Prints one JSON line: per measured part the median time,
TFLOP/s and the fraction of the 157.3 TFLOP/s fp32 MFMA peak.

    python tools/sent_cnn_bench.py [--iters 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmonkey_amd import autodiff as F   # noqa: E402
from neuralmonkey_amd import ops             # noqa: E402

PEAK = 157.3e12


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    bsz, slen, e, seg, depth = 128, 250, 128, 5, 4
    filters = list(zip(range(1, 9), (200, 200, 250, 250, 300, 300, 300, 300)))
    width = sum(n for _, n in filters)
    sp, _ = ops.conv1d_pool_shape(slen, seg)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(bsz, slen, e, device=dev, generator=g)
    ws = [torch.randn(w, e, n, device=dev, generator=g) / (w * e) ** 0.5 for w, n in filters]
    bs = [torch.randn(n, device=dev, generator=g) * 0.1 for _, n in filters]
    pooled = torch.empty(bsz, sp, width, device=dev)
    arg = torch.empty(bsz, sp, width, dtype=torch.int32, device=dev)
    dpooled = torch.randn(bsz, sp, width, device=dev, generator=g)
    dz = torch.empty(bsz, slen, width, device=dev)
    dx = torch.empty(bsz, slen, e, device=dev)
    dws = [torch.empty_like(w) for w in ws]
    dbs = [torch.empty_like(b) for b in bs]
    wsp = torch.empty(ops.conv1d_wgrad_workspace_floats(bsz, slen, e, ws), device=dev)
    conv_flop = 2.0 * bsz * slen * e * sum(w * n for w, n in filters)
    res = {"shape": {"B": bsz, "S": slen, "E": e, "filters": filters, "segment": seg, "highway": [depth, width]}}

    def put(name, ms, flop):
        res[name] = {"ms": round(ms, 4), "tflops": round(flop / ms / 1e9, 2), "of_peak": round(flop / ms / 1e9 / 157.3, 3)}

    put("conv_fwd", timed(lambda: ops.conv1d_pool_fwd(x, ws, bs, seg, pooled, arg), args.iters), conv_flop)
    put("conv_dgrad", timed(lambda: ops.conv1d_pool_bwd(x, ws, seg, pooled, arg, dpooled, dz, dx=dx), args.iters),
        conv_flop)
    t_all = timed(lambda: ops.conv1d_pool_bwd(x, ws, seg, pooled, arg, dpooled, dz, dweights=dws, dbiases=dbs,
                                              accumulate_params=False, workspace=wsp), args.iters)
    t_route = timed(lambda: ops.conv1d_pool_bwd(x, ws, seg, pooled, arg, dpooled, dz), args.iters)
    put("conv_wgrad", t_all - t_route, conv_flop)       # conv_wgrad_mfma + conv_wgrad_reduce + conv_bias_grad
    res["conv_route_ms"] = round(t_route, 4)

    rows = bsz * sp
    hx = torch.randn(rows, width, device=dev, generator=g)
    hw = [torch.randn(width, width, device=dev, generator=g) / width ** 0.5 for _ in range(2)]
    hb = [torch.full((width,), -1.0, device=dev) for _ in range(2)]

    class _Ctx:
        device = dev
        session = type("Session", (), {})()

        def __init__(self):
            self.bufs = {}

        def buffer(self, key, shape, dtype=torch.float32, zero=False):
            t = self.bufs.get(key)
            if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
                t = self.bufs[key] = torch.empty(shape, dtype=dtype, device=dev)
            if zero:
                ops.zero(t)
            return t
    ctx = _Ctx()
    grads = [torch.zeros_like(t) for t in (hw[0], hb[0], hw[1], hb[1])]

    def hw_fwd(record):
        tape = F.Tape(ctx, "hw", recording=record)
        xv = F.Var(hx, None, record)
        params = [F.Var(t, gr, record) for t, gr in zip((hw[0], hb[0], hw[1], hb[1]), grads)]
        return tape, F.highway(tape, xv, *params)

    hw_flop = 2.0 * 2 * rows * width * width
    put("highway_fwd", timed(lambda: hw_fwd(False), args.iters), hw_flop)
    dy = torch.randn(rows, width, device=dev, generator=g)

    def hw_fb():
        tape, y = hw_fwd(True)
        y.grad = dy
        tape.backward()
    put("highway_fwd_bwd", timed(hw_fb, args.iters), 3 * hw_flop)
    res["highway_bwd"] = {"ms": round(res["highway_fwd_bwd"]["ms"] - res["highway_fwd"]["ms"], 4)}

    def encoder_front():
        ops.conv1d_pool_fwd(x, ws, bs, seg, pooled, arg)
        tapes = []
        for _ in range(depth):
            tape, y = hw_fwd(True)
            tapes.append((tape, y))
        for tape, y in reversed(tapes):
            y.grad = dy
            tape.backward()
        ops.conv1d_pool_bwd(x, ws, seg, pooled, arg, dpooled, dz, dx=dx, dweights=dws, dbiases=dbs,
                            accumulate_params=False, workspace=wsp)
    put("cnn_highway_fwd_bwd", timed(encoder_front, max(5, args.iters // 2)), 3 * conv_flop + depth * 3 * hw_flop)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
