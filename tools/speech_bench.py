"""HIP-event timings of the speech front end's kernels (csrc/nm_speech.hip) on a ragged batch: --utterances recordings of
2 to 6 seconds at --rate Hz, MFCC with two delta orders (the features of the reference's tests/ctc.ini).

  frames          nm_speech_frames over the batch: one workgroup per frame
  deltas          one nm_speech_deltas launch (one delta order)
  stream_read     nm_prof_stream_read of the batch's samples: the yardstick, a plain float4 read of what ``frames`` reads
  many            ``SpeechFeaturesPreprocessor.many`` end to end on the host clock: concatenation, the copies to the
                  device, the launches, the copy back and the split into arrays

Medians of --iters launches between two HIP events after three warm-up launches.

    python tools/speech_bench.py [--iters 50] [--utterances 64] [--rate 16000] [--out profiles/speech_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmonkey_amd import _lib, ops                                              # noqa: E402
from neuralmonkey_amd.processors.speech import FEATURE_TYPES, SpeechFeaturesPreprocessor, frame_count  # noqa: E402
from neuralmonkey_amd.readers.audio_reader import Audio                             # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--rate", type=int, default=16000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/speech_bench.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    audios = [Audio(args.rate, (rng.standard_normal(int(n)) * 3000).astype(np.int16))
              for n in rng.integers(2 * args.rate, 6 * args.rate, args.utterances)]
    pre = SpeechFeaturesPreprocessor("mfcc", 2)
    tab = pre.tables(args.rate)
    sample_off = np.concatenate([[0], np.cumsum([len(a.data) for a in audios])]).astype(np.int64)
    frame_off = np.concatenate([[0], np.cumsum([frame_count(len(a.data), tab.frame_len, tab.frame_step)
                                                for a in audios])]).astype(np.int64)
    wav = torch.from_numpy(np.concatenate([a.data for a in audios]).astype(np.float32)).to(dev)
    d_samples, d_frames = torch.from_numpy(sample_off).to(dev), torch.from_numpy(frame_off).to(dev)
    out = torch.empty((int(frame_off[-1]), 39), device=dev)
    tables = tab.on_device(dev)
    sink = torch.zeros(2048, device=dev)
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    res = {"rate": args.rate, "utterances": args.utterances, "samples": int(sample_off[-1]), "frames": int(frame_off[-1]),
           "nfft": tab.nfft,
           "frames_kernel": timed(lambda: ops.speech_frames(wav, d_samples, d_frames, tab.frame_len, tab.frame_step,
                                                            tab.nfft, tab.preemph, tables, FEATURE_TYPES["mfcc"], 13,
                                                            True, out), args.iters),
           "deltas_kernel": timed(lambda: ops.speech_deltas(out, d_frames, 13, 0, 2), args.iters),
           "stream_read": timed(lambda: lib.nm_prof_stream_read(stream, wav.data_ptr(), wav.numel() * 4,
                                                                sink.data_ptr()), args.iters)}
    walls = []
    for _ in range(7):
        torch.cuda.synchronize()
        start = time.perf_counter()
        pre.many(audios)
        walls.append((time.perf_counter() - start) * 1e3)
    walls.sort()
    res["many"] = {"median_ms": round(walls[len(walls) // 2], 3), "min_ms": round(walls[0], 3), "max_ms": round(walls[-1], 3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
