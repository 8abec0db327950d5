"""HIP-event timings of the streaming attention entry points (csrc/nm_sdp_stream.hip).

  long      nm_sdp_stream_fwd (with row_max / row_sum, no weights) and nm_sdp_stream_bwd (its three launches together)
            at B = 16, H = 8, dh = 64, Tq = Tk = T in 256, 1024, 4096, causal, no key mask, no dropout
  beside    at T = 128 and T = 150 the same two calls beside nm_sdp_attn_fwd (with its weights output, which its
            backward reads) and nm_sdp_attn_bwd on the same operands: the resident matrix-core kernels at 128, the
            resident wave-per-query kernels at 150.  The two routes' ctx and gradients are compared first.

Median (and min, max) of --reps calls between two HIP events after three warm-up calls.  ``tflops`` counts the
products the algorithm needs over the full Tq x Tk rectangle (forward 2, dQ 3, dK / dV 4 products of
2 B H Tq Tk dh each), ``of_peak`` is that over the 157.3 TFLOP/s of the exact-fp32 matrix instruction.  The split
of the backward into its launches comes from a kernel trace of this same script, taken in a run of its own.

    python tools/sdp_stream_bench.py [--reps 20] [--out profiles/sdp_stream_events.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmonkey_amd import ops             # noqa: E402
from tools.mbr_bench import events             # noqa: E402

BATCH, HEADS, DH = 16, 8, 64
PEAK = 157.3e12


def operands(t, dev):
    gen = torch.Generator(device=dev).manual_seed(t)
    d = HEADS * DH
    return [torch.randn(BATCH, t, d, device=dev, generator=gen) for _ in range(4)]        # q, k, v, dctx


def stream_calls(t, q, k, v, g):
    ctx, grads = torch.empty_like(q), [torch.empty_like(x) for x in (q, k, v)]
    rmax, rsum = (torch.empty(BATCH, HEADS, t, device=q.device) for _ in range(2))
    ws = ops.sdp_stream_workspace(BATCH, HEADS, t, q.device)
    fwd = lambda: ops.sdp_stream_fwd(q, k, v, None, HEADS, ctx, None, rmax, rsum, causal=True)
    bwd = lambda: ops.sdp_stream_bwd(q, k, v, None, ctx, rmax, rsum, g, HEADS, *grads, ws, causal=True)
    return fwd, bwd, [ctx] + grads


def resident_calls(t, q, k, v, g):
    ctx, grads = torch.empty_like(q), [torch.empty_like(x) for x in (q, k, v)]
    w, de = (torch.empty(BATCH, HEADS, t, t, device=q.device) for _ in range(2))
    fwd = lambda: ops.sdp_attn_fwd(q, k, v, None, HEADS, ctx, w, causal=True)
    bwd = lambda: ops.sdp_attn_bwd(q, k, v, None, w, g, HEADS, *grads, de, causal=True)
    return fwd, bwd, [ctx] + grads


def timed(route, t, fwd, bwd, reps):
    flop = 2.0 * BATCH * HEADS * t * t * DH
    r = {"route": route, "B": BATCH, "H": HEADS, "dh": DH, "T": t}
    for name, fn, products in (("fwd", fwd, 2), ("bwd", bwd, 7)):
        median, spread = events(fn, reps)
        r[name + "_us"], r[name + "_min_max_us"] = median, spread
        r[name + "_tflops"] = round(products * flop / median / 1e6, 2)
        r[name + "_of_peak"] = round(products * flop / (median * 1e-6) / PEAK, 3)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lengths", type=int, nargs="*", default=[256, 1024, 4096])
    ap.add_argument("--beside", type=int, nargs="*", default=[128, 150])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    results = []
    for t in args.lengths:
        fwd, bwd, _ = stream_calls(t, *operands(t, dev))
        results.append(timed("stream", t, fwd, bwd, args.reps))
    for t in args.beside:
        x = operands(t, dev)
        s_fwd, s_bwd, s_out = stream_calls(t, *x)
        r_fwd, r_bwd, r_out = resident_calls(t, *x)
        for fn in (s_fwd, s_bwd, r_fwd, r_bwd):
            fn()
        diffs = [float((a - b).abs().max()) for a, b in zip(s_out, r_out)]
        assert max(diffs) < 1e-4, diffs
        results.append(timed("resident", t, r_fwd, r_bwd, args.reps))
        results.append(dict(timed("stream", t, s_fwd, s_bwd, args.reps),
                            max_abs_diff_ctx_dq_dk_dv=[float("%.1e" % x) for x in diffs]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
