"""Time the truncated sampling step (nm_sample_step) at B = 128, V = 32000 with HIP events.

  n = 1, 8, 64 samples per sentence (128, 1024, 8192 rows of N(0, 1) logits), four settings each: nothing truncated
  (k = 0, p = 1), top-k (k = 40), nucleus (p = 0.9), both;
  the yardstick in the same run: what an untruncated draw costs without the entry, nm_row_stats (for the
  log-probability) + nm_gumbel_argmax over the same rows.

Warm: the call repeated back to back on the same logits.  Cold: a 1 GiB buffer is overwritten before every timed call, so
nothing of the logits is left in the caches.  Median of ``--reps`` (30) calls.  Each time is also given as a multiple of
the time ONE read of the rows' fp32 logits takes at the 8 TB/s HBM peak DESIGN.md uses.

    python tools/sample_bench.py [--out FILE.json]"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
from neuralmonkey_amd import ops  # noqa: E402

HBM_PEAK = 8e12                     # bytes / s
dev = torch.device("cuda:0")
B, V = 128, 32000
SETTINGS = [(0, 1.0), (40, 1.0), (0, 0.9), (40, 0.9)]
flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)


def _events(fn, n, cold):
    times = []
    for _ in range(n):
        if cold:
            flush.fill_(1.0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def _state(n):
    torch.manual_seed(n)
    rows = B * n
    i32 = lambda: torch.zeros(rows, dtype=torch.int32, device=dev)
    f32 = lambda: torch.zeros(rows, device=dev)
    return {"logits": torch.randn((rows, V), device=dev), "salt": torch.full((1,), 12345, dtype=torch.int32, device=dev),
            "fin": i32(), "lps": f32(), "lens": i32(), "sym": i32(), "lp": f32(), "kept": i32(), "fin2": i32(),
            "lps2": f32(), "lens2": i32(), "rmax": f32(), "rlse": f32(), "allfin": torch.ones(1, dtype=torch.int32, device=dev)}


def _sample(s, top_k, top_p):
    ops.sample_step(s["logits"], s["salt"], 7, 2, s["fin"], s["lps"], s["lens"], s["sym"], s["lp"], s["kept"], s["fin2"],
                    s["lps2"], s["lens2"], top_k=top_k, top_p=top_p, all_finished=s["allfin"])


def _yardstick(s):
    ops.row_stats(s["logits"], s["rmax"], s["rlse"], None)
    ops.gumbel_argmax(s["logits"], 12352, s["sym"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    results = []

    def record(name, n, fn, extra=None):
        one_read = B * n * V * 4 / HBM_PEAK * 1e6
        fn()
        fn()
        torch.cuda.synchronize()
        warm, cold = _events(fn, args.reps, False), _events(fn, args.reps, True)
        r = {"kernel": name, "n": n, "rows": B * n, "warm_us": round(warm[0], 1),
             "warm_min_max_us": [round(warm[1], 1), round(warm[2], 1)], "cold_us": round(cold[0], 1),
             "cold_min_max_us": [round(cold[1], 1), round(cold[2], 1)], "one_read_at_8TBs_us": round(one_read, 1),
             "warm_over_one_read": round(warm[0] / one_read, 2), "cold_over_one_read": round(cold[0] / one_read, 2)}
        r.update(extra or {})
        results.append(r)
        print(json.dumps(r), flush=True)

    for n in (1, 8, 64):
        s = _state(n)
        record("nm_row_stats + nm_gumbel_argmax", n, lambda: _yardstick(s))
        for top_k, top_p in SETTINGS:
            record("nm_sample_step", n, lambda: _sample(s, top_k, top_p), {"top_k": top_k, "top_p": top_p})
            torch.cuda.synchronize()
            results[-1]["mean_kept"] = round(float(s["kept"].float().mean()), 1)
        del s
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"B": B, "V": V, "hbm_peak_bytes_per_s": HBM_PEAK, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
