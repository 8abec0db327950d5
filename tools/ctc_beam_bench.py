"""HIP-event timings of CTC prefix beam search (nm_ctc_beam_search, csrc/nm_ctc_beam.hip) beside greedy CTC decoding
(nm_ctc_greedy) on the same logits, at the two shapes of tools/ctc_bench.py:

  speech        B = 32, T = 800 frames, K = 41 classes: the frame scan, a chain of T dependent frames per sentence
  translation   B = 128, T = 50, K = 32001: the row pass, bound by the one read of the [T*B, K] logits

Prints one JSON line and, with --out, writes it to a file.  Per shape and beam size: the median time of a call (row pass
+ frame scan + backtrack), the time per frame (call time / T), the row pass's algorithmic bytes (4 T B K read,
4 T B (2 M + 2) written) over the call time as a fraction of the 8 TB/s HBM peak -- the whole call's time, so a lower
bound on the row pass's own share -- and greedy decoding's time.

    python tools/ctc_beam_bench.py [--iters 20] [--out profiles/ctc_beam_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmonkey_amd import ops             # noqa: E402
from ctc_bench import HBM_PEAK, timed        # noqa: E402

SHAPES = {"speech": (32, 800, 41, (1, 8, 16, 64)), "translation": (128, 50, 32001, (8, 64))}


def bench(name, dev, iters):
    bsz, steps, k, beams = SHAPES[name]
    rng = np.random.default_rng(1)
    logits = torch.tensor((rng.standard_normal((steps, bsz, k)) * 3.0).astype(np.float32), device=dev)
    flen = torch.full((bsz,), steps, dtype=torch.int32, device=dev)
    tokens = torch.empty(bsz, steps, dtype=torch.int32, device=dev)
    out_len = torch.empty(bsz, dtype=torch.int32, device=dev)
    score = torch.empty(bsz, device=dev)
    res = {"B": bsz, "T": steps, "K": k,
           "greedy_ms": round(timed(lambda: ops.ctc_greedy(logits, flen, True, 2, tokens, out_len), iters), 4)}
    for beam in beams:
        ms = timed(lambda: ops.ctc_beam_search(logits, flen, beam, True, 2, tokens, out_len, score), iters)
        short = min(beam + 1, k - 1)
        row_bytes = 4.0 * steps * bsz * (k + 2 * short + 2)
        res["beam_{}".format(beam)] = {"ms": round(ms, 4), "per_frame_us": round(1e3 * ms / steps, 3),
                                       "row_pass_bytes": row_bytes,
                                       "hbm_fraction_of_call": round(row_bytes / (ms * 1e-3) / HBM_PEAK, 4),
                                       "mean_emitted": float(out_len.float().mean().cpu())}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ctc_beam_bench.py measures on a GPU; none is visible")
    line = json.dumps({name: bench(name, torch.device("cuda:0"), args.iters) for name in sorted(SHAPES)})
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
