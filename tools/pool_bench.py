"""HIP-event timings of the kernels of the sentence-level heads (csrc/nm_pool.hip) against the same expressions in
torch-ROCm, and of the softmax over time against two transposes around the library's ``attn_softmax`` (which
normalises along the contiguous axis), on the same inputs:

  pooling   masked max / average over time of [128, 50, 1024] and [128, 50, 600] states (lengths 1..50), forward and
            backward; algorithmic bytes = the states read once (forward; max backward reads them again) and the gradient
            written once, over the time, as a fraction of the 8 TB/s HBM peak.  NB both inputs (26 and 15 MB) fit the
            256 MB Infinity Cache: the fraction says how far the kernel is from the HBM roofline, not where its bytes
            came from.
  softmax   [128, 50, 8] energies: nm_time_softmax_fwd / _bwd in the natural layout against transpose -> attn_softmax
            -> transpose, and against torch.

Medians of --iters runs between two HIP events after three warm-up runs; the two sides of every comparison are checked
for agreement before anything is timed.

    python tools/pool_bench.py [--iters 20] [--out profiles/pool_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmonkey_amd import ops             # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = [(128, 50, 1024), (128, 50, 600)]
HEADS = 8


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


def chained(fn, iters, reps=20):
    """``reps`` launches back to back between ONE event pair, per launch: what a launch costs inside a step, without the
    dispatch and event latency that a lone launch between two events mostly measures at these sizes."""
    def many():
        for _ in range(reps):
            fn()
    return timed(many, iters) / reps


def inputs(bsz, steps, width, dev, seed):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, steps + 1, size=bsz)
    lengths[0] = steps
    mask = (np.arange(steps)[None, :] < lengths[:, None]).astype(np.float32)
    x = rng.standard_normal((bsz, steps, width)).astype(np.float32)
    dout = rng.standard_normal((bsz, width)).astype(np.float32)
    return torch.tensor(x, device=dev), torch.tensor(mask, device=dev), torch.tensor(dout, device=dev)


def bench_pool(shape, dev, iters):
    bsz, steps, d = shape
    x, mask, dout = inputs(bsz, steps, d, dev, d)
    m3 = mask[:, :, None]
    out, ties = torch.empty(bsz, d, device=dev), torch.empty(bsz, d, dtype=torch.int32, device=dev)
    dx = torch.empty_like(x)
    res = {"shape": list(shape)}
    state_bytes = 4.0 * bsz * steps * d

    def torch_max():
        return torch.amax(x * m3 + 1e-15 * (1 - m3), dim=1)

    def torch_avg():
        return (x * m3).sum(dim=1) / (m3.sum(dim=1) + 1e-8)

    def torch_max_bwd():
        p = x * m3 + 1e-15 * (1 - m3)
        eq = (p == torch.amax(p, dim=1, keepdim=True)).float()
        return m3 * eq * (dout[:, None, :] / eq.sum(dim=1, keepdim=True))

    def torch_avg_bwd():
        return m3 * (dout / (m3.sum(dim=1) + 1e-8))[:, None, :] * torch.ones_like(x)
    ops.pool_fwd("max", x, mask, out, ties)
    agree = {"max": float((out - torch_max()).abs().max().cpu())}
    ops.pool_bwd("max", dout, mask, dx, x=x, out=out, ties=ties)
    agree["max_bwd"] = float((dx - torch_max_bwd()).abs().max().cpu())
    ops.pool_fwd("avg", x, mask, out)
    agree["avg"] = float((out - torch_avg()).abs().max().cpu())
    ops.pool_bwd("avg", dout, mask, dx)
    agree["avg_bwd"] = float((dx - torch_avg_bwd()).abs().max().cpu())
    ops.pool_fwd("max", x, mask, out, ties)
    t = {"max_fwd_ms": timed(lambda: ops.pool_fwd("max", x, mask, out, ties), iters),
         "max_bwd_ms": timed(lambda: ops.pool_bwd("max", dout, mask, dx, x=x, out=out, ties=ties), iters),
         "avg_fwd_ms": timed(lambda: ops.pool_fwd("avg", x, mask, out), iters),
         "avg_bwd_ms": timed(lambda: ops.pool_bwd("avg", dout, mask, dx), iters),
         "torch_max_fwd_ms": timed(torch_max, iters), "torch_max_bwd_ms": timed(torch_max_bwd, iters),
         "torch_avg_fwd_ms": timed(torch_avg, iters), "torch_avg_bwd_ms": timed(torch_avg_bwd, iters)}
    t.update({"max_fwd_chain_ms": chained(lambda: ops.pool_fwd("max", x, mask, out, ties), iters),
              "max_bwd_chain_ms": chained(lambda: ops.pool_bwd("max", dout, mask, dx, x=x, out=out, ties=ties), iters),
              "avg_fwd_chain_ms": chained(lambda: ops.pool_fwd("avg", x, mask, out), iters),
              "avg_bwd_chain_ms": chained(lambda: ops.pool_bwd("avg", dout, mask, dx), iters)})
    res.update({k: round(v, 4) for k, v in t.items()})
    for name, nbytes in (("max_fwd", state_bytes), ("avg_fwd", state_bytes), ("max_bwd", 2 * state_bytes),
                         ("avg_bwd", state_bytes)):
        res[name + "_bytes"] = nbytes
        res[name + "_hbm_fraction"] = round(nbytes / (t[name + "_ms"] * 1e-3) / HBM_PEAK, 4)
        res[name + "_chain_hbm_fraction"] = round(nbytes / (t[name + "_chain_ms"] * 1e-3) / HBM_PEAK, 4)
        res[name + "_speedup_vs_torch"] = round(t["torch_" + name + "_ms"] / t[name + "_ms"], 2)
    res["agreement"] = agree
    return res


def bench_softmax(dev, iters, bsz=128, steps=50, heads=HEADS):
    e, mask, _ = inputs(bsz, steps, heads, dev, 7)
    dw = torch.tensor(np.random.default_rng(8).standard_normal((bsz, steps, heads)).astype(np.float32), device=dev)
    w, s, de = torch.empty_like(e), torch.empty_like(e), torch.empty_like(e)
    z = torch.empty(bsz, heads, device=dev)
    wt, det = torch.empty(bsz, heads, steps, device=dev), torch.empty(bsz, heads, steps, device=dev)

    def mine():
        ops.time_softmax_fwd(e, mask, w, s, z)

    def mine_bwd():
        ops.time_softmax_bwd(dw, s, z, mask, de)

    def transposed():
        et = e.transpose(1, 2).contiguous()
        ops.attn_softmax_fwd(et.view(bsz * heads, steps), mask, wt.view(bsz * heads, steps), bsz, heads)
        return wt.transpose(1, 2).contiguous()

    def transposed_bwd():
        # (nm_attn_softmax_bwd finds a row's sentence as row % B: the rows are laid out [H, B])
        et = e.permute(2, 0, 1).contiguous()
        dwt = dw.permute(2, 0, 1).contiguous()
        ops.attn_softmax_bwd(dwt.view(heads * bsz, steps), et.view(heads * bsz, steps), mask,
                             det.view(heads * bsz, steps), bsz)
        return det.view(heads, bsz, steps).permute(1, 2, 0).contiguous()

    def in_torch():
        sm = torch.softmax(e, dim=1) * mask[:, :, None]
        return sm / (sm.sum(dim=1, keepdim=True) + 1e-8)
    mine()
    mine_bwd()
    res = {"shape": [bsz, steps, heads],
           "agreement": {"transposed_attn_softmax": float((w - transposed()).abs().max().cpu()),
                         "torch": float((w - in_torch()).abs().max().cpu())}}
    res["agreement"]["transposed_attn_softmax_bwd"] = float((de - transposed_bwd()).abs().max().cpu())
    t = {"time_softmax_fwd_ms": timed(mine, iters), "time_softmax_bwd_ms": timed(mine_bwd, iters),
         "transposed_attn_softmax_fwd_ms": timed(transposed, iters), "torch_fwd_ms": timed(in_torch, iters)}
    t["transposed_attn_softmax_bwd_ms"] = timed(transposed_bwd, iters)
    t.update({"time_softmax_fwd_chain_ms": chained(mine, iters), "time_softmax_bwd_chain_ms": chained(mine_bwd, iters),
              "transposed_attn_softmax_fwd_chain_ms": chained(transposed, iters),
              "transposed_attn_softmax_bwd_chain_ms": chained(transposed_bwd, iters)})
    res.update({k: round(v, 4) for k, v in t.items()})
    res["fwd_speedup_vs_transposed"] = round(t["transposed_attn_softmax_fwd_ms"] / t["time_softmax_fwd_ms"], 2)
    res["fwd_speedup_vs_torch"] = round(t["torch_fwd_ms"] / t["time_softmax_fwd_ms"], 2)
    res["bwd_speedup_vs_transposed"] = round(t["transposed_attn_softmax_bwd_ms"] / t["time_softmax_bwd_ms"], 2)
    res["fwd_chain_speedup_vs_transposed"] = round(t["transposed_attn_softmax_fwd_chain_ms"]
                                                   / t["time_softmax_fwd_chain_ms"], 2)
    res["bwd_chain_speedup_vs_transposed"] = round(t["transposed_attn_softmax_bwd_chain_ms"]
                                                   / t["time_softmax_bwd_chain_ms"], 2)
    nbytes = 4.0 * bsz * steps * heads
    res["fwd_bytes"] = 3 * nbytes
    res["fwd_hbm_fraction"] = round(3 * nbytes / (t["time_softmax_fwd_ms"] * 1e-3) / HBM_PEAK, 5)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pool_bench.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    res = {"x".join(str(n) for n in shape): bench_pool(shape, dev, args.iters) for shape in SHAPES}
    res["softmax"] = bench_softmax(dev, args.iters)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
