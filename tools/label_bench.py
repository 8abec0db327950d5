"""HIP-event timings of the labelling-head kernel (csrc/nm_label.hip) against the three vocabulary-row calls it
replaces, on the same inputs in the same library:

  fused   ops.label_rows: loss + gradient (in place) + argmax + masked labels + log-probabilities, ONE launch
  three   ops.xent (loss + gradient in place: nm_xent) + ops.row_stats (max, log-sum-exp, argmax: nm_row_stats)
          + ops.log_softmax_from_stats (nm_log_softmax), each timed alone and all three back to back

rows = 6400 (B * T of a tagging batch) at K = 43 (the reference's tag set) and K = 1024 (the packed kernel's widest
row), plus the register-count steps in between with --sweep.  Medians of --iters runs between two HIP events after three
warm-up runs.  Both sides overwrite their logits with the gradient, so later iterations read gradients instead of
logits: the work per element does not depend on the values.  Algorithmic bytes of the fused call: the logits read once,
gradient and log-probabilities written once (3 * 4 * rows * K) plus 24 bytes per row; over the time, as a fraction of
the 8 TB/s HBM peak.

    python tools/label_bench.py [--iters 20] [--sweep] [--out profiles/label_bench.json]
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
ROWS = 6400
CLASSES = [43, 1024]
SWEEP = [43, 64, 128, 256, 512, 1024]


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


def bench(k, dev, iters, rows=ROWS):
    rng = np.random.default_rng(k)
    host = (rng.standard_normal((rows, k)) * 2.0).astype(np.float32)
    tgt = rng.integers(0, k, size=rows).astype(np.int32)
    tgt[rng.random(rows) < 0.2] = 0                                  # a fifth of the positions are <pad>
    x_fused, x_xent, x_stats = (torch.tensor(host, device=dev) for _ in range(3))
    targets = torch.tensor(tgt, device=dev)
    weights = torch.tensor((tgt != 0).astype(np.float32), device=dev)
    mask = torch.ones(rows, device=dev)
    loss, loss3 = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    lp, lp3 = torch.empty(rows, k, device=dev), torch.empty(rows, k, device=dev)
    amax, amax3 = (torch.empty(rows, dtype=torch.int32, device=dev) for _ in range(2))
    labels = torch.empty(rows, dtype=torch.int32, device=dev)
    rmax, rlse = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    scale = torch.tensor([1.0 / max(1, int((tgt != 0).sum()))], device=dev)

    def fused():
        ops.label_rows(x_fused, targets, 0, scale, True, loss, lp, amax, mask, 2, labels)

    def xent():
        ops.xent(x_xent, targets, weights, loss3, scale, True)

    def stats():
        ops.row_stats(x_stats, rmax, rlse, amax3)

    def logsm():
        ops.log_softmax_from_stats(x_stats, rmax, rlse, lp3)

    def three():
        xent()
        stats()
        logsm()

    # the two sides agree before anything is timed
    fused()
    three()
    torch.cuda.synchronize()
    agree = {"loss": float((loss - loss3).abs().max().cpu()), "grad": float((x_fused - x_xent).abs().max().cpu()),
             "logprobs": float((lp - lp3).abs().max().cpu()), "argmax_equal": bool(torch.equal(amax, amax3))}
    t = {"fused_ms": timed(fused, iters), "xent_ms": timed(xent, iters), "row_stats_ms": timed(stats, iters),
         "log_softmax_ms": timed(logsm, iters), "three_back_to_back_ms": timed(three, iters),
         "fused_train_only_ms": timed(lambda: ops.label_rows(x_fused, targets, 0, scale, True, loss), iters),
         "fused_labels_only_ms": timed(lambda: ops.label_rows(x_fused, None, 0, None, False, None, None, amax, mask, 2,
                                                              labels), iters)}
    res = {"rows": rows, "K": k}
    res.update({name: round(v, 4) for name, v in t.items()})
    res["three_sum_ms"] = round(t["xent_ms"] + t["row_stats_ms"] + t["log_softmax_ms"], 4)
    res["speedup_vs_sum"] = round(res["three_sum_ms"] / t["fused_ms"], 2)
    res["speedup_vs_back_to_back"] = round(t["three_back_to_back_ms"] / t["fused_ms"], 2)
    res["algorithmic_bytes"] = 12.0 * rows * k + 24.0 * rows
    res["hbm_fraction_fused"] = round(res["algorithmic_bytes"] / (t["fused_ms"] * 1e-3) / HBM_PEAK, 4)
    res["agreement"] = agree
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweep", action="store_true", help="every register-count step of the packed kernel")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/label_bench.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    res = {"K{}".format(k): bench(k, dev, args.iters) for k in (SWEEP if args.sweep else CLASSES)}
    res["max_classes"] = ops.label_rows_max_classes()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
