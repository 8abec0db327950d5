"""HIP-event timings of the two kernels of MBR decoding (nm_mbr_pairwise, nm_mbr_select; csrc/nm_mbr.hip) beside the host
path they replace: the NumPy ``sentence_gleu`` / ``sentence_bleu`` over the same tiled pairs.

  grid      B in {16, 64} sentences, n in {8, 64} samples, T in {32, 128} positions, over a small vocabulary (8 words:
            n-grams repeat, the clipping works) and a realistic one (32 000 words); the samples of a sentence share
            70 % of their positions with a common sentence, and every sample ends at a random place in the second half
            of its T positions, <pad> behind </s>
  kernel    median (and min, max) of --reps launches between two HIP events after three warm-up launches
  host      the NumPy utility on the FIRST --host-pairs tiled pairs of the same batch (wall clock), scaled by
            B * n * n / pairs timed: the whole batch would take minutes at the larger sizes.  ``host_scaled_ms`` says so
            by its name; ``host_measured_ms`` and ``host_pairs`` are what was measured

The device's utilities of the timed host pairs are checked against the host's (GLEU bit-equal, BLEU within 1 float32
ulp) before anything is timed.

    python tools/mbr_bench.py [--reps 20] [--host-pairs 128] [--out profiles/mbr_events.json]
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
from neuralmonkey_amd.decoders.mbr_decoder import tile_pairs      # noqa: E402
from neuralmonkey_amd.trainers.self_critical_objective import sentence_bleu, sentence_gleu      # noqa: E402

PAD, END = 0, 2
HOST = {"gleu": sentence_gleu, "bleu": sentence_bleu}


def events(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return round(times[len(times) // 2], 1), [round(times[0], 1), round(times[-1], 1)]


def samples(bsz, n, steps, words, seed):
    rng = np.random.default_rng(seed)
    tok = rng.integers(3, 3 + words, (steps, bsz, n)).astype(np.int32)
    base = np.broadcast_to(rng.integers(3, 3 + words, (steps, bsz, 1)).astype(np.int32), tok.shape)
    kept = rng.random(tok.shape) < 0.7                            # samples of one sentence resemble each other
    tok[kept] = base[kept]
    end =rng.integers(steps // 2, steps + 1, (bsz, n))           # == steps: the sample never ended
    t = np.arange(steps)[:, None, None]
    tok[t == end[None]] = END
    tok[t > end[None]] = PAD
    return tok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-pairs", type=int, default=128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    results = []
    for words in (8, 32000):
        for bsz in (16, 64):
            for n in (8, 64):
                for steps in (32, 128):
                    tok = samples(bsz, n, steps, words, seed=bsz * 1000 + n * 10 + steps)
                    d_tok = torch.tensor(tok, device=dev)
                    utilities = torch.empty((bsz, n, n), dtype=torch.float32, device=dev)
                    expected = torch.empty((bsz, n), dtype=torch.float32, device=dev)
                    best = torch.empty((bsz,), dtype=torch.int32, device=dev)
                    chosen = torch.empty((steps, bsz), dtype=torch.int32, device=dev)
                    pairs = bsz * n * n
                    timed_pairs = min(args.host_pairs, pairs)
                    references, hypotheses = (a[:, :timed_pairs] for a in tile_pairs(tok))
                    for kind in ("gleu", "bleu"):
                        got = ops.mbr_pairwise(kind, d_tok, END, out=utilities).cpu().numpy().reshape(-1)[:timed_pairs]
                        t0 = time.perf_counter()
                        want = HOST[kind](references, hypotheses)
                        host_ms = (time.perf_counter() - t0) * 1e3
                        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()
                        assert ulps <= (1 if kind == "bleu" else 0), (kind, ulps)
                        median, spread = events(lambda kind=kind: ops.mbr_pairwise(kind, d_tok, END, out=utilities),
                                                args.reps)
                        r = {"kernel": "nm_mbr_pairwise", "kind": kind, "words": words, "B": bsz, "n": n, "T": steps,
                             "pairs": pairs, "wavefronts": bsz * n * (n + 1) // 2, "us": median, "min_max_us": spread,
                             "host_pairs": timed_pairs, "host_measured_ms": round(host_ms, 2),
                             "host_scaled_ms": round(host_ms * pairs / timed_pairs, 1)}
                        r["host_scaled_over_kernel"] = round(r["host_scaled_ms"] * 1e3 / median, 0)
                        results.append(r)
                        print(json.dumps(r), flush=True)
                    median, spread = events(lambda: ops.mbr_select(utilities, d_tok, expected, best, chosen), args.reps)
                    r = {"kernel": "nm_mbr_select", "words": words, "B": bsz, "n": n, "T": steps, "us": median,
                         "min_max_us": spread}
                    results.append(r)
                    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
