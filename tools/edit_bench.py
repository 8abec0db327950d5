"""HIP-event timings of nm_edit_pairwise (csrc/nm_edit.hip) at B = 64 sentences with n = 64 samples of
T = 32, 128 and 1024 positions, beside the path the same utility takes when ``MBRDecoder`` does not recognise it: one
call of the NumPy function over the tiled pairs on the host, between two copies.

  samples   over 30 words; the samples of a sentence share 70 % of their positions with a common sentence, and every
            sample ends at a random place in the second half of its T positions, <pad> behind </s>
  kernel    median (and min, max) of --reps launches between two HIP events after three warm-up launches
  host      ``MBRDecoder(utility=<a wrapper the decoder does not know>).outputs`` on the samples of ONE sentence cut to
            --host-samples samples (wall clock around the call and a synchronisation: copy out, the NumPy function on
            the n * n tiled pairs, copy back, nm_mbr_select; the second of two calls), scaled by 64 * 64 * 64 / pairs
            timed: the whole batch would take some twenty minutes at T = 1024.  ``host_scaled_ms`` says so by its
            name and is an order of magnitude, not a measurement; ``host_measured_ms`` and ``host_pairs`` are what was
            measured

The device's utilities of the timed host pairs are checked against the host's, bit for bit, before anything is timed.

    python tools/edit_bench.py [--reps 20] [--host-samples 8] [--out profiles/edit_events.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmonkey_amd import ops, synthetic             # noqa: E402
from neuralmonkey_amd.decoders import MBRDecoder, SamplingDecoder      # noqa: E402
from neuralmonkey_amd.decoders.sampling_decoder import SamplingOutput      # noqa: E402
from neuralmonkey_amd.runtime import RunContext             # noqa: E402
from neuralmonkey_amd.trainers.self_critical_objective import sentence_edit_accuracy, sentence_neg_wer      # noqa: E402
from tools.mbr_bench import END, events, samples             # noqa: E402

HOST = {"accuracy": sentence_edit_accuracy, "neg_wer": sentence_neg_wer}
BATCH, SAMPLES = 64, 64


def host_route(model, d_tok, kind):
    """(utilities [1, n, n], milliseconds) of MBRDecoder.outputs over the given samples with a utility it sends to the
    host."""
    steps, bsz, n = d_tok.shape
    sampler = SamplingDecoder(name="bench_sampler_{}_{}".format(kind, steps), parent_decoder=model.decoder,
                              max_steps=steps, num_samples=n)
    decoder = MBRDecoder("bench_mbr_{}_{}".format(kind, steps), sampler,
                         utility=lambda references, hypotheses: HOST[kind](references, hypotheses))
    drawn = SamplingOutput(d_tok, torch.zeros((bsz, n), device=d_tok.device),
                           torch.zeros((bsz, n), dtype=torch.int32, device=d_tok.device),
                           torch.zeros((bsz, n), dtype=torch.int32, device=d_tok.device))
    for _ in range(2):                 # the first call creates the session's buffers and loads nm_mbr_select: not timed
        ctx = RunContext(model.tf_manager.sessions[0], {})
        ctx.memo[sampler.outputs.key] = drawn
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = decoder.outputs(ctx)
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3
    return out.utilities.cpu().numpy(), host_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-samples", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = synthetic.build_translation_model(vocab_src=30, vocab_tgt=40, emb=8, rnn=8, max_len=6, beam_size=0,
                                              max_steps=4, device="cuda:0")
    results = []
    for steps in (32, 128, 1024):
        tok = samples(BATCH, SAMPLES, steps, 30, seed=steps)
        d_tok = torch.tensor(tok, device=dev)
        utilities = torch.empty((BATCH, SAMPLES, SAMPLES), dtype=torch.float32, device=dev)
        few = args.host_samples
        d_few = torch.tensor(np.ascontiguousarray(tok[:, :1, :few]), device=dev)
        for kind in ("accuracy", "neg_wer"):
            got = ops.edit_pairwise(kind, d_tok, END, out=utilities).cpu().numpy()[:1, :few, :few]
            want, host_ms = host_route(model, d_few, kind)
            assert got.tobytes() == want.tobytes(), (kind, steps)
            median, spread = events(lambda kind=kind: ops.edit_pairwise(kind, d_tok, END, out=utilities), args.reps)
            pairs = BATCH * SAMPLES * SAMPLES
            r = {"kernel": "nm_edit_pairwise", "kind": kind, "B": BATCH, "n": SAMPLES, "T": steps, "pairs": pairs,
                 "distances": BATCH * SAMPLES * (SAMPLES - 1) // 2, "us": median, "min_max_us": spread,
                 "host_pairs": few * few, "host_measured_ms": round(host_ms, 2),
                 "host_scaled_ms": round(host_ms * pairs / (few * few), 1)}
            r["host_scaled_over_kernel"] = float("%.1e" % (r["host_scaled_ms"] * 1e3 / median))     # two digits at most
            results.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
