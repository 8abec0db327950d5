"""HIP-event timings of the CTC kernels (csrc/nm_ctc.hip) at two shapes, next to torch's own
``log_softmax`` + ``ctc_loss`` (+ backward) of the installed torch-ROCm on the same inputs (the comparison runs in this
tool only, never in the product):

  speech        B = 32, T = 800 frames, L ~ 60 labels, K = 41 classes: a latency-bound chain of T dependent steps
  translation   B = 128, T = 50, L <= 25, K = 32001: bound by the traffic over the [T*B, K] logits

Prints one JSON line and, with --out, writes it to a file (profiles/ctc_bench.json).  Per shape: the median time of
loss forward, forward + gradient (out of place, as torch's) and greedy decoding; the per-frame latency of the
recursion (forward time / T); the algorithmic bytes of forward + gradient (the logits read for the row log-sum-exps,
read again and written once for the gradient: 3 K T B floats, plus alpha and beta written and read) over the time, as
a fraction of the 8 TB/s HBM peak; torch's times; whether the two agree on the loss.

    python tools/ctc_bench.py [--iters 20] [--out profiles/ctc_bench.json] [--only-ours]
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
SHAPES = {"speech": (32, 800, 60, 41), "translation": (128, 50, 25, 32001)}


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


def make(name, dev):
    bsz, steps, lmax, k = SHAPES[name]
    rng = np.random.default_rng(1)
    logits = torch.tensor((rng.standard_normal((steps, bsz, k)) * 2.0).astype(np.float32), device=dev)
    lens = rng.integers(max(1, lmax - 10), lmax + 1, size=bsz).astype(np.int32)
    labels = np.zeros((bsz, lmax), np.int32)
    for b in range(bsz):
        labels[b, :lens[b]] = rng.integers(0, k - 1, size=lens[b])
    frame_len = np.full(bsz, steps, np.int32)
    return logits, labels, lens, frame_len


def bench(name, dev, iters, with_torch):
    bsz, steps, lmax, k = SHAPES[name]
    logits, labels, lens, frame_len = make(name, dev)
    lab, lab_len = torch.tensor(labels, device=dev), torch.tensor(lens, device=dev)
    flen = torch.tensor(frame_len, device=dev)
    loss, total = torch.empty(bsz, device=dev), torch.empty(1, device=dev)
    grad = torch.empty_like(logits)
    tokens = torch.empty(bsz, steps, dtype=torch.int32, device=dev)
    out_len = torch.empty(bsz, dtype=torch.int32, device=dev)
    ws = ops.ctc_workspace(bsz, steps, lmax, dev)

    def fwd():
        return ops.ctc_loss_fwd(logits, lab, lab_len, flen, True, loss, total, ws)

    def fwd_bwd():
        ops.ctc_loss_bwd(logits, lab, lab_len, flen, grad, fwd())

    t_fwd, t_both = timed(fwd, iters), timed(fwd_bwd, iters)
    t_greedy = timed(lambda: ops.ctc_greedy(logits, flen, True, 2, tokens, out_len, ws), iters)
    states = 2 * lmax + 1
    algo_bytes = 4.0 * (3 * steps * bsz * k + 4 * steps * bsz * states)
    res = {"B": bsz, "T": steps, "L": lmax, "K": k, "fwd_ms": round(t_fwd, 4), "fwd_bwd_ms": round(t_both, 4),
           "greedy_ms": round(t_greedy, 4), "chain_length": steps, "per_frame_us": round(1e3 * t_fwd / steps, 3),
           "algorithmic_bytes": algo_bytes, "hbm_fraction_fwd_bwd": round(algo_bytes / (t_both * 1e-3) / HBM_PEAK, 4),
           "greedy_hbm_fraction": round(4.0 * steps * bsz * k / (t_greedy * 1e-3) / HBM_PEAK, 4)}
    fwd_bwd()
    ours = float(total.cpu()[0])
    res["loss_sum"] = ours
    if with_torch:
        x = logits.clone().requires_grad_(True)
        targets = torch.tensor(np.concatenate([labels[b, :lens[b]] for b in range(bsz)]), device=dev, dtype=torch.long)
        in_len, tg_len = flen.long(), lab_len.long()

        def t_fwd_fn():
            with torch.no_grad():
                return torch.nn.functional.ctc_loss(torch.log_softmax(x, -1), targets, in_len, tg_len, blank=k - 1,
                                                    reduction="sum", zero_infinity=True)

        def t_both_fn():
            x.grad = None
            torch.nn.functional.ctc_loss(torch.log_softmax(x, -1), targets, in_len, tg_len, blank=k - 1,
                                         reduction="sum", zero_infinity=True).backward()

        res["torch_fwd_ms"] = round(timed(t_fwd_fn, iters), 4)
        res["torch_fwd_bwd_ms"] = round(timed(t_both_fn, iters), 4)
        res["torch_greedy_argmax_ms"] = round(timed(lambda: x.detach().argmax(-1), iters), 4)
        theirs = float(t_fwd_fn().cpu())
        t_both_fn()
        res["torch_loss_sum"] = theirs
        res["loss_rel_diff"] = abs(ours - theirs) / abs(theirs)
        res["grad_max_diff"] = float((x.grad - grad).abs().max().cpu())
        res["speedup_fwd_bwd"] = round(res["torch_fwd_bwd_ms"] / t_both, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-ours", action="store_true", help="skip torch's ctc_loss (kernel-trace runs)")
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ctc_bench.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    res = {name: bench(name, dev, args.iters, not args.only_ours) for name in sorted(SHAPES)
           if args.shape in (None, name)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
