"""HIP-event timings of the reward kernels of self-critical training (csrc/nm_reward.hip) beside the NumPy functions
they replace on the hot path (trainers/self_critical_objective.py: ``sentence_bleu`` / ``sentence_gleu``, what the
reference runs behind ``tf.py_func``), at the size of a training step: B = 128 sentences, T = 50 positions, references
and hypotheses of ragged lengths over a vocabulary of 30 000 with a fifth of the hypothesis copied from the reference.

  kernel    median of --iters runs between two HIP events after three warm-up runs, and the same per launch with 20
            launches between one event pair (what a launch costs inside a step)
  host      wall clock of the NumPy function on the same arrays -- without the two device-to-host copies and the
            host-to-device copy the py_func path adds around it

The two sides are checked for agreement (GLEU bit-equal, BLEU within 1 float32 ulp) before anything is timed.

    python tools/reward_bench.py [--iters 20] [--out profiles/reward_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmonkey_amd import ops             # noqa: E402
from neuralmonkey_amd.trainers.self_critical_objective import sentence_bleu, sentence_gleu      # noqa: E402

END = 2


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
    def many():
        for _ in range(reps):
            fn()
    return timed(many, iters) / reps


def sentences(bsz, steps, vocab, seed):
    rng = np.random.default_rng(seed)
    ref = rng.integers(4, vocab, (steps, bsz)).astype(np.int32)
    hyp = rng.integers(4, vocab, (steps, bsz)).astype(np.int32)
    copied = rng.random((steps, bsz)) < 0.2
    hyp[copied] = ref[copied]
    for arr in (ref, hyp):
        lengths = rng.integers(steps // 2, steps + 1, bsz)
        for b, n in enumerate(lengths):
            if n < steps:
                arr[n, b] = END
                arr[n + 1:, b] = 0
    return ref, hyp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    ref, hyp = sentences(args.batch, args.steps, 30000, 7)
    d_ref, d_hyp = torch.tensor(ref, device=dev), torch.tensor(hyp, device=dev)
    out = torch.empty(args.batch, dtype=torch.float32, device=dev)
    lines = []
    for kind, host_fn in (("bleu", sentence_bleu), ("gleu", sentence_gleu)):
        got = ops.sentence_reward(kind, d_ref, d_hyp, END, out=out).cpu().numpy()
        want = host_fn(ref, hyp)
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()
        assert ulps <= (1 if kind == "bleu" else 0), (kind, ulps)
        run = lambda kind=kind: ops.sentence_reward(kind, d_ref, d_hyp, END, out=out)
        host = []
        for _ in range(5):
            t0 = time.perf_counter()
            host_fn(ref, hyp)
            host.append((time.perf_counter() - t0) * 1e3)
        lines.append({"what": "nm_sentence_reward " + kind, "batch": args.batch, "steps": args.steps,
                      "kernel_ms": timed(run, args.iters), "kernel_chained_ms": chained(run, args.iters),
                      "numpy_host_ms": sorted(host)[len(host) // 2], "mean_reward": float(want.mean())})
    mask = torch.tensor((np.asarray(hyp) != 0).astype(np.int32), device=dev)
    reward, baseline = torch.rand(args.batch, device=dev), torch.rand(args.batch, device=dev)
    w = torch.empty((args.steps, args.batch), dtype=torch.float32, device=dev)
    scale, inv = torch.empty(1, device=dev), torch.empty(1, device=dev)
    run = lambda: ops.reinforce_weights(reward, baseline, mask, 0.5, w, scale, inv)
    r, b, m = reward.cpu().numpy(), baseline.cpu().numpy(), mask.cpu().numpy()
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        _ = (-(r - b))[None, :] * m.astype(np.float32), np.float32(0.5) / np.float32(m.sum())
        host.append((time.perf_counter() - t0) * 1e3)
    lines.append({"what": "nm_reinforce_weights", "batch": args.batch, "steps": args.steps,
                  "kernel_ms": timed(run, args.iters), "kernel_chained_ms": chained(run, args.iters),
                  "numpy_host_ms": sorted(host)[len(host) // 2]})
    for line in lines:
        print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as handle:
            for line in lines:
                handle.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
