"""HIP-event timings of nm_chrf_reward and nm_chrf_pairwise (csrc/nm_chrf.hip) at a training step's and an
MBR decoding's sizes -- B = 128 sentences of T = 50 positions, and n = 64 samples of each -- beside the route the same
``SentenceChrF`` takes when its callers do not find the tensors on the device: the arrays to the host, the object's
``__call__`` there, the result back.

  vocabulary 32 000 words of 1 to 12 lower-case letters (a third of them BPE pieces "x@@"), joined: streams of some
            150 to 300 characters
  samples   ``tools/mbr_bench.samples``: the samples of a sentence share 70 % of their positions with a common sentence,
            and every sample ends at a random place in the second half of its T positions, <pad> behind </s>
  kernel    median (and min, max) of --reps launches between two HIP events after three warm-up launches
  host      wall clock around copy out, ``SentenceChrF.__call__``, copy back and a synchronisation.  The 128 pairs of the
            reward are timed whole.  Of the 128 * 64 * 64 pairs of the utilities the first --host-pairs are timed and
            scaled: ``host_scaled_ms`` says so by its name and is an order of magnitude, not a measurement;
            ``host_measured_ms`` and ``host_pairs`` are what was measured

The device's scores of the timed host pairs are checked against the host's (2^-23) before anything is timed.

    python tools/chrf_bench.py [--reps 20] [--host-pairs 256] [--out profiles/chrf_events.json]
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
from neuralmonkey_amd.trainers.self_critical_objective import SentenceChrF      # noqa: E402
from neuralmonkey_amd.vocabulary import Vocabulary      # noqa: E402
from tools.mbr_bench import END, events, samples             # noqa: E402

BATCH, SAMPLES, STEPS, WORDS = 128, 64, 50, 32000


def vocabulary(seed=0):
    rng = np.random.default_rng(seed)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    return Vocabulary(["".join(rng.choice(letters, rng.integers(1, 13))) + ("@@" if k % 3 == 0 else "")
                       for k in range(WORDS - 4)])


def host_route(chrf, references, hypotheses, device):
    """(scores on the device, milliseconds): the callers' host branch on device tensors [T, N]."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = chrf(references.cpu().numpy(), hypotheses.cpu().numpy().astype(np.int64))
    out = torch.from_numpy(np.ascontiguousarray(host)).to(device)
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-pairs", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    chrf = SentenceChrF(vocabulary(), join_subwords=True)
    table = chrf.device_table(dev)
    tok = samples(BATCH, SAMPLES, STEPS, WORDS - 3, seed=1)
    d_tok = torch.tensor(tok, device=dev)
    results = []

    # the reward of a training step: sample 0 of every sentence against sample 1
    references, hypotheses = d_tok[:, :, 1].contiguous(), d_tok[:, :, 0].contiguous()
    reward = torch.empty(BATCH, dtype=torch.float32, device=dev)
    got = ops.chrf_reward(references, hypotheses, END, table, chrf.n, chrf.beta, out=reward).cpu().numpy()
    want, host_ms = host_route(chrf, references, hypotheses, dev)
    assert np.abs(got - want.cpu().numpy()).max() <= 2.0 ** -23
    median, spread = events(lambda: ops.chrf_reward(references, hypotheses, END, table, chrf.n, chrf.beta, out=reward),
                            args.reps)
    results.append({"kernel": "nm_chrf_reward", "B": BATCH, "T": STEPS, "pairs": BATCH, "us": median,
                    "min_max_us": spread, "host_pairs": BATCH, "host_measured_ms": round(host_ms, 2),
                    "max_word_chars": table.max_word_chars, "mean_score": round(float(got.mean()), 4)})
    print(json.dumps(results[-1]), flush=True)

    # the utilities of MBR decoding
    utilities = torch.empty((BATCH, SAMPLES, SAMPLES), dtype=torch.float32, device=dev)
    got = ops.chrf_pairwise(d_tok, END, table, chrf.n, chrf.beta, out=utilities).cpu().numpy().reshape(-1)
    pairs, timed = BATCH * SAMPLES * SAMPLES, args.host_pairs
    few = [torch.tensor(np.ascontiguousarray(a[:, :timed]), device=dev) for a in tile_pairs(tok[:, :1])]
    want, host_ms = host_route(chrf, few[0], few[1], dev)
    assert np.abs(got[:timed] - want.cpu().numpy()).max() <= 2.0 ** -23
    median, spread = events(lambda: ops.chrf_pairwise(d_tok, END, table, chrf.n, chrf.beta, out=utilities), args.reps)
    r = {"kernel": "nm_chrf_pairwise", "B": BATCH, "n_samples": SAMPLES, "T": STEPS, "pairs": pairs,
         "wavefronts": BATCH * SAMPLES * (SAMPLES - 1) // 2, "us": median, "min_max_us": spread, "host_pairs": timed,
         "host_measured_ms": round(host_ms, 2), "host_scaled_ms": round(host_ms * pairs / timed, 1)}
    r["host_scaled_over_kernel"] = float("%.1e" % (r["host_scaled_ms"] * 1e3 / median))     # two digits at most
    results.append(r)
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
