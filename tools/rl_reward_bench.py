"""Both routes of ``ReinforceObjective.rewards`` (trainers/rl_trainer.py) on one MI355X at the size of a training step:
B = 128 sentences, S = 2 samples, T = 50 positions, ragged references and sampled symbols over a vocabulary of 30 000
with a fifth of the hypothesis copied from the reference; GLEU and BLEU.

  device   ``nm_eval_sentence_score`` (csrc/nm_rl.hip): KERNEL time -- the S launches of a step between two HIP events,
           median of --iters after three warm-up runs, and the same per step with 20 steps between one event pair --
           and, like for like with the host route, WALL CLOCK around the S calls of a step ending in a synchronise
           (the Python-side enqueue included)
  host     the reference's route: both arrays to the host, indices -> words -> the BPE join -> the evaluator once per
           sentence, the result back to the device; wall clock around the S calls of a step, ending in a synchronise

The two routes are checked for agreement (GLEU equal, BLEU within 1 float32 ulp) before anything is timed.

    python tools/rl_reward_bench.py [--iters 20] [--out profiles/rl_reward_bench.json]

``--pieces`` runs the same sizes over a BPE-style vocabulary of the same 30 000 entries, two fifths of them continuation
pieces ("w17@@"), where equal words are not equal indices:

  joined   ``nm_eval_joined_sentence_score`` (csrc/nm_subword.hip), timed like ``device`` above
  host     the reference's route on the same piece vocabulary
  whole    ``nm_eval_sentence_score`` on the same index arrays read over the whole-word vocabulary: the kernel the new
           one stands beside (other words, so other scores: a time to compare, not a result)

All three routes are checked before anything is timed: joined against host on the pieces, and the joined kernel given
the whole-word vocabulary's table against the whole-word kernel, bit for bit.

    python tools/rl_reward_bench.py --pieces [--iters 20] [--out profiles/rl_reward_pieces_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reward_bench import chained, sentences, timed                           # noqa: E402
from neuralmonkey_amd import ops, synthetic                                    # noqa: E402
from neuralmonkey_amd.evaluators.bleu import BLEUEvaluator                     # noqa: E402
from neuralmonkey_amd.evaluators.gleu import GLEUEvaluator                     # noqa: E402
from neuralmonkey_amd.trainers.rl_trainer import ReinforceObjective, device_piece_table   # noqa: E402
from neuralmonkey_amd.vocabulary import Vocabulary                             # noqa: E402


def wall_clock(fn, runs):
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return sorted(times)[len(times) // 2], [min(times), max(times)]


def pieces_leg(args, model, d_ref, d_hyps, out):
    whole_words = model.decoder.vocabulary
    words = list(whole_words.index_to_word)[4:]
    pieces = Vocabulary([w + "@@" if i % 5 < 2 else w for i, w in enumerate(words)])
    assert len(pieces) == len(whole_words)
    whole_table = device_piece_table(whole_words, d_ref.device)
    lines = []
    for kind, evaluator in (("gleu", GLEUEvaluator()), ("bleu", BLEUEvaluator())):
        model.decoder.vocabulary = whole_words
        whole = ReinforceObjective(model.decoder, evaluator, sample_size=args.samples)
        assert whole.device_reward() == (kind, 4)

        def step(objective, vocabulary):
            model.decoder.vocabulary = vocabulary
            for s in range(args.samples):
                objective.rewards(None, d_ref, d_hyps[s], out[s])
        joined = ReinforceObjective(model.decoder, evaluator, sample_size=args.samples)
        on_host = ReinforceObjective(model.decoder, lambda h, r, fn=evaluator: fn(h, r), sample_size=args.samples)
        model.decoder.vocabulary = pieces
        assert joined.device_reward() is None and joined.joined_device_reward() == (kind, 4)
        assert on_host.joined_device_reward() is None
        # agreement, before anything is timed
        step(joined, pieces)
        got = out.cpu().numpy().copy()
        step(on_host, pieces)
        want = out.cpu().numpy().copy()
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()
        assert ulps <= (1 if kind == "bleu" else 0), (kind, ulps)
        step(whole, whole_words)
        index_scores = out.cpu().numpy().copy()
        for s in range(args.samples):
            ops.eval_joined_sentence_score(kind, 4, d_ref, d_hyps[s], whole_table, out=out[s])
        assert out.cpu().numpy().tobytes() == index_scores.tobytes(), kind
        host, host_spread = wall_clock(lambda: step(on_host, pieces), 5)
        wall, wall_spread = wall_clock(lambda: step(joined, pieces), max(args.iters, 5))
        lines.append({"what": "ReinforceObjective.rewards " + kind + " over pieces", "batch": args.batch,
                      "steps": args.steps, "samples": args.samples, "continuation_pieces": 0.4,
                      "joined_ms_per_step": timed(lambda: step(joined, pieces), args.iters),
                      "joined_chained_ms_per_step": chained(lambda: step(joined, pieces), args.iters),
                      "joined_wall_ms_per_step": wall, "joined_wall_ms_spread": wall_spread,
                      "host_ms_per_step": host, "host_ms_spread": host_spread,
                      "whole_word_ms_per_step": timed(lambda: step(whole, whole_words), args.iters),
                      "whole_word_chained_ms_per_step": chained(lambda: step(whole, whole_words), args.iters),
                      "mean_reward": float(want.mean()), "mean_reward_whole_words": float(index_scores.mean())})
    model.decoder.vocabulary = whole_words
    return lines


def words_leg(args, model, d_ref, d_hyps, out):
    lines = []
    for kind, evaluator in (("gleu", GLEUEvaluator()), ("bleu", BLEUEvaluator())):
        on_device = ReinforceObjective(model.decoder, evaluator, sample_size=args.samples)
        on_host = ReinforceObjective(model.decoder, lambda h, r, fn=evaluator: fn(h, r), sample_size=args.samples)
        assert on_device.device_reward() == (kind, 4) and on_host.device_reward() is None

        def step(objective):
            for s in range(args.samples):
                objective.rewards(None, d_ref, d_hyps[s], out[s])
        step(on_device)
        got = out.cpu().numpy().copy()
        step(on_host)
        want = out.cpu().numpy().copy()
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()
        assert ulps <= (1 if kind == "bleu" else 0), (kind, ulps)
        host = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(on_host)
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
        wall = []
        for _ in range(max(args.iters, 5)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(on_device)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        lines.append({"what": "ReinforceObjective.rewards " + kind, "batch": args.batch, "steps": args.steps,
                      "samples": args.samples, "device_ms_per_step": timed(lambda: step(on_device), args.iters),
                      "device_chained_ms_per_step": chained(lambda: step(on_device), args.iters),
                      "device_wall_ms_per_step": sorted(wall)[len(wall) // 2], "device_wall_ms_spread": [min(wall), max(wall)],
                      "host_ms_per_step": sorted(host)[len(host) // 2], "host_ms_spread": [min(host), max(host)],
                      "mean_reward": float(want.mean())})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pieces", action="store_true", help="the leg over a BPE-style vocabulary")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev, vocab = "cuda:0", 30000
    model = synthetic.build_translation_model(vocab_src=200, vocab_tgt=vocab, emb=8, rnn=8, max_len=args.steps,
                                              device=dev)
    ref, _ = sentences(args.batch, args.steps, vocab, 7)
    hyps = [sentences(args.batch, args.steps, vocab, 7 + s)[1] for s in range(args.samples)]
    for hyp in hyps:                                   # a fifth of every sample copied from the one reference
        copied = np.random.default_rng(3).random(hyp.shape) < 0.2
        hyp[copied] = ref[copied]
    d_ref = torch.tensor(ref, device=dev)
    d_hyps = [torch.tensor(h, device=dev) for h in hyps]
    out = torch.empty((args.samples, args.batch), dtype=torch.float32, device=dev)
    lines = (pieces_leg if args.pieces else words_leg)(args, model, d_ref, d_hyps, out)
    for line in lines:
        print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as handle:
            for line in lines:
                handle.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
