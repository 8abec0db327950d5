"""What the image reader's device pipeline (csrc/nm_imgread.hip) costs on one chunk of --images decoded images of the
sizes of the reference's tests/data/str (grey word images, 31 rows, 50 to 400 columns), read the way tests/str.ini reads
them: resized to 256 x 32 with BILINEAR in mode F.  Each part on its own:

  tables          the host's part: geometry and Pillow's coefficient tables in float64 (``ChunkPlan``), host clock, the
                  tables' cache emptied before every repetition (every size is new)
  tables_cached   the same with every table already in the cache (every size has been seen)
  upload          the five arrays (pixels, offsets, geometry, bounds, coefficients) to the device, host clock, synchronised
  rows_kernel     nm_imgread_rows between two HIP events
  cols_kernel     nm_imgread_cols between two HIP events
  copy_back       the [N, 32, 256, 1] float32 result to the host, host clock, synchronised
  pillow          where Pillow is importable: ``Image.fromarray(pixels).convert("F").resize((256, 32), BILINEAR)`` and
                  ``np.array`` of it for the same images, one by one on the host (decoding is in neither figure)

Medians of --iters repetitions after three warm-up ones.

    python tools/image_reader_bench.py [--iters 50] [--images 64] [--out profiles/image_reader_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmonkey_amd import ops                                                     # noqa: E402
from neuralmonkey_amd.readers.image_reader import ChunkPlan, identity_table, plan_image, resample_table  # noqa: E402


def summary(times, unit):
    times = sorted(times)
    return {"median_" + unit: round(times[len(times) // 2], 3), "min_" + unit: round(times[0], 3),
            "max_" + unit: round(times[-1], 3)}


def events(fn, iters):
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
    return summary(times, "us")


def wall(fn, iters):
    for _ in range(3):
        fn()
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        start = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - start) * 1e6)
    return summary(times, "us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/image_reader_bench.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    images = [rng.integers(0, 256, (31, int(w)), dtype=np.uint8) for w in rng.integers(50, 400, args.images)]

    def make():
        return ChunkPlan(images, [plan_image(p.shape[1], p.shape[0], 256, 32, True, True, False) for p in images], "F",
                         256, 32)

    def make_cold():
        resample_table.cache_clear()
        identity_table.cache_clear()
        return make()
    plan = make()
    names = ("src", "offs", "geom", "bounds", "coef")

    def upload():
        return {n: torch.from_numpy(getattr(plan, n)).to(dev) for n in names}
    d = upload()
    scratch = torch.empty(plan.scratch_elems, dtype=torch.float32, device=dev)
    out = torch.empty((args.images, 32, 256, 1), dtype=torch.float32, device=dev)
    res = {"images": args.images, "source_pixels": int(plan.offs[0, -1]), "target": "256x32 F, BILINEAR",
           "upload_bytes": int(sum(getattr(plan, n).nbytes for n in names)),
           "tables": wall(make_cold, args.iters), "tables_cached": wall(make, args.iters),
           "upload": wall(upload, args.iters),
           "rows_kernel": events(lambda: ops.imgread_rows(d["src"], d["offs"], d["geom"], d["bounds"], d["coef"],
                                                          plan.target, 256, plan.max_rows, scratch), args.iters),
           "cols_kernel": events(lambda: ops.imgread_cols(scratch, d["offs"], d["geom"], d["bounds"], d["coef"],
                                                          plan.target, out), args.iters),
           "copy_back": wall(lambda: out.cpu().numpy(), args.iters)}
    try:
        from PIL import Image
    except ImportError:
        res["pillow"] = None
    else:
        res["pillow"] = wall(lambda: [np.array(Image.fromarray(p).convert("F").resize((256, 32), Image.BILINEAR))
                                      for p in images], args.iters)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
