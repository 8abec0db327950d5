"""HIP-event timings of the supervised-attention kernels (csrc/nm_align.hip) at the headline size -- attention weights
[T = 50, B = 128, S = 50], a fed alignment [128, 50, 50] -- and of the training step with and without the objective.

Kernels (medians of --iters launches between two HIP events after three warm-up launches, the buffers warm in cache as
they are inside a step, where the attention's own kernels have just written them):

  xent_loss       nm_align_xent, dw = NULL: reads the weights and the labels once (2 * 4 * T*B*S bytes)
  xent_grad       nm_align_xent adding into dw: + the gradient read and written (4 * 4 * T*B*S bytes)
  softmax         nm_align_softmax: weights read, [B, T, S] written
  stream_read     nm_prof_stream_read of 2 * 4 * T*B*S bytes: the yardstick, a plain float4 read of what xent_loss reads
  empty_launch    nm_align_xent with T = 0, which returns before it launches: the host side of a call alone

Step (--step): the headline translation model (vocabulary 32000, hidden 512, 128 sentences of 50 tokens, the hand-
scheduled path) trained with the cost objective alone -- the launch sequence of a tree without this feature -- and with
an alignment objective of weight 0.5 beside it; the two alternate, --repeats windows of --inner steps each, host clock
around a window that ends in a device synchronise.

    python tools/align_bench.py [--iters 50] [--step] [--out profiles/align_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmonkey_amd import _lib, ops, synthetic             # noqa: E402

STEPS, BATCH, SRC = 50, 128, 50


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
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return {"median_us": round(times[len(times) // 2], 2), "min_us": round(times[0], 2), "max_us": round(times[-1], 2)}


def kernels(dev, iters):
    rng = np.random.default_rng(1)
    w = rng.random((STEPS, BATCH, SRC)).astype(np.float32)
    w /= w.sum(axis=2, keepdims=True)
    label = (rng.random((BATCH, STEPS, SRC)) < 0.05).astype(np.float32)
    label /= np.maximum(label.sum(axis=2, keepdims=True), 1.0)
    wd, td = torch.tensor(w, device=dev), torch.tensor(label, device=dev)
    pad = torch.ones(STEPS, BATCH, device=dev)
    loss, dw = torch.empty(STEPS, BATCH, device=dev), torch.zeros(STEPS, BATCH, SRC, device=dev)
    out = torch.empty(BATCH, STEPS, SRC, device=dev)
    scale = torch.tensor([1e-3], device=dev)
    both = torch.cat([wd.reshape(-1), td.reshape(-1)])
    sink = torch.zeros(2048, device=dev)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    empty = torch.empty(0, BATCH, SRC, device=dev)
    elems = STEPS * BATCH * SRC
    res = {"shape": [STEPS, BATCH, SRC],
           "xent_loss": timed(lambda: ops.align_xent(wd, td, pad, loss), iters),
           "xent_grad": timed(lambda: ops.align_xent(wd, td, pad, loss, scale, dw=dw, accumulate=True), iters),
           "softmax": timed(lambda: ops.align_softmax(wd, out), iters),
           "stream_read": timed(lambda: lib.nm_prof_stream_read(stream, both.data_ptr(), both.numel() * 4,
                                                                sink.data_ptr()), iters),
           "empty_launch": timed(lambda: ops.align_xent(empty, td, pad[:0], loss[:0]), iters)}
    res["xent_loss"]["bytes"], res["xent_grad"]["bytes"] = 8 * elems, 16 * elems
    res["softmax"]["bytes"], res["stream_read"]["bytes"] = 8 * elems, 8 * elems
    return res


def step_times(dev, repeats, inner):
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    from neuralmonkey_amd.decoders import WordAlignmentDecoder
    from neuralmonkey_amd.trainers import CrossEntropyTrainer
    m = synthetic.build_translation_model(device=dev, seed=1234, beam_size=0, with_trainer=False)
    synthetic.load_baseline_weights(m.tf_manager.sessions[0].store)
    wad = WordAlignmentDecoder(m.encoder, m.decoder, "ali", "aligner")
    trainers = {"cost_only": CrossEntropyTrainer(decoders=[m.decoder], l2_weight=1e-8, clip_norm=1.0),
                "with_alignment": CrossEntropyTrainer(decoders=[m.decoder, wad], decoder_weights=[1.0, 0.5],
                                                      l2_weight=1e-8, clip_norm=1.0)}
    src, tgt = synthetic.synthetic_ids(1234, BATCH, SRC, STEPS, 32000)
    rng = np.random.default_rng(2)
    ali = []
    for _ in range(BATCH):
        mat = (rng.random((STEPS, SRC)) < 0.05).astype(np.float32)
        ali.append(mat / np.maximum(mat.sum(axis=1, keepdims=True), 1.0))
    ds = Dataset("bench", {"source": src, "target": tgt, "ali": ali}, BatchingScheme(batch_size=BATCH))
    windows = {name: [] for name in trainers}
    for rep in range(repeats + 1):                                     # (the first round is warm-up)
        for name, trainer in trainers.items():
            torch.cuda.synchronize()
            start = time.perf_counter()
            for _ in range(inner):
                res = m.tf_manager.execute(ds, trainer.feedables, [trainer], train=True)[0]
            torch.cuda.synchronize()
            if rep:
                windows[name].append((time.perf_counter() - start) / inner * 1e3)
    losses = {k: float(v) for k, v in res.losses.items()}
    out = {"inner": inner, "last_losses": losses}
    for name, vals in windows.items():
        vals.sort()
        out[name] = {"median_ms": round(vals[len(vals) // 2], 4), "min_ms": round(vals[0], 4), "max_ms": round(vals[-1], 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step", action="store_true", help="also time the training step with and without the objective")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/align_bench.py measures on a GPU; none is visible")
    res = {"kernels": kernels(torch.device("cuda:0"), args.iters)}
    if args.step:
        res["step"] = step_times("cuda:0", args.repeats, args.inner)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
