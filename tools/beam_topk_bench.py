"""Time the beam step kernels at B = 128, V = 32000 with HIP events.

  nm_beam_topk_step (k = 5, the headline beam; NM_BEAM_NS overrides its slice count) and nm_row_stats, as before;
  nm_beam_topk_step at k = 16 and nm_beam_topk_step_wide at k = 16, 32, 64 in the same run, the wide entry in both
  conventions: statistics given (one counting pass + the slices that reach the k-th best) and computed by the entry.

Warm: the call repeated back to back on the same logits.  Cold: a 1 GiB buffer is overwritten before every timed call, so
nothing of the logits is left in the caches.  Each time is also given as a multiple of the time ONE read of the
B*k*V fp32 logits takes at the 8 TB/s HBM peak DESIGN.md uses.  The last figure per wide run is the share of the
(row, slice) workgroups whose slice the second pass read again.

    python tools/beam_topk_bench.py [--out FILE.json]"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
from neuralmonkey_amd import ops  # noqa: E402

HBM_PEAK = 8e12                     # bytes / s
dev = torch.device("cuda:0")
B, V = 128, 32000
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


def _state(k):
    torch.manual_seed(k)
    rows = B * k
    s = {"logits": torch.randn((rows, V), device=dev),
         "rmax": torch.empty(rows, device=dev), "rlse": torch.empty(rows, device=dev),
         "lps": -torch.rand((B, k), device=dev) * 20,
         "lens": torch.randint(0, 30, (B, k), dtype=torch.int32, device=dev),
         "fin": torch.zeros((B, k), dtype=torch.int32, device=dev),
         "penalty": ops.length_penalty_table(64, 0.6, dev),
         "scores": torch.empty((B, k), device=dev),
         "ws": ops.beam_workspace(B, k, V, dev), "allfin": torch.ones(1, dtype=torch.int32, device=dev)}
    s["word"], s["beam"], s["src"], s["lens2"], s["fin2"] = (torch.empty((B, k), dtype=torch.int32, device=dev)
                                                             for _ in range(5))
    s["lps2"] = torch.empty((B, k), device=dev)
    ops.row_stats(s["logits"], s["rmax"], s["rlse"], None)
    return s


def _narrow(s, k):
    ops.beam_topk_step(s["logits"], B, k, s["rmax"], s["rlse"], s["lps"], s["lens"], s["fin"], s["penalty"], 2,
                       s["scores"], s["word"], s["beam"], s["lps2"], s["lens2"], s["fin2"], s["src"], s["ws"], s["allfin"])


def _wide(s, k, given):
    kw = {"rmax_in": s["rmax"], "rlse_in": s["rlse"]} if given else {}
    ops.beam_topk_step_wide(s["logits"], B, k, s["lps"], s["lens"], s["fin"], s["penalty"], 2, s["scores"], s["word"],
                            s["beam"], s["lps2"], s["lens2"], s["fin2"], s["src"], s["ws"],
                            None if given else s["rmax"], None if given else s["rlse"], s["allfin"], **kw)


def _reread_share(s, k):
    """(row, slice) workgroups whose highest bin reaches the sentence's threshold bin, from the workspace layout of
    csrc/nm_logits.hip (wide_layout, k > 16): header 16 ints, then k*ns list lengths, then k*ns highest bins."""
    if k <= 16:
        return None
    ns = min(8, (V + 8191) // 8192)
    nwg = k * ns
    stride = (ops._lib.load().nm_beam_workspace_bytes(B, k, V) - 256) // 4 // B
    w = s["ws"].view(torch.int32)[:B * stride].view(B, stride).cpu()
    smax = w[:, 16 + ((nwg + 1) & ~1):16 + ((nwg + 1) & ~1) + nwg]
    return float((smax >= w[:, 1:2]).float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    results = []

    def record(name, k, fn, s):
        one_read = B * k * V * 4 / HBM_PEAK * 1e6
        fn()
        fn()
        torch.cuda.synchronize()
        warm, cold = _events(fn, args.reps, False), _events(fn, args.reps, True)
        r = {"kernel": name, "k": k, "warm_us": round(warm[0], 1), "warm_min_max_us": [round(warm[1], 1), round(warm[2], 1)],
             "cold_us": round(cold[0], 1), "cold_min_max_us": [round(cold[1], 1), round(cold[2], 1)],
             "one_read_at_8TBs_us": round(one_read, 1), "warm_over_one_read": round(warm[0] / one_read, 2),
             "cold_over_one_read": round(cold[0] / one_read, 2)}
        if name.startswith("nm_beam_topk_step_wide"):
            r["slices_read_again"] = _reread_share(s, k)
        results.append(r)
        print(json.dumps(r))

    s = _state(5)
    record("nm_beam_topk_step", 5, lambda: _narrow(s, 5), s)
    record("nm_row_stats", 5, lambda: ops.row_stats(s["logits"], s["rmax"], s["rlse"], None), s)
    for k in (16, 32, 64):
        s = _state(k)
        if k == 16:
            record("nm_beam_topk_step", 16, lambda: _narrow(s, 16), s)
        record("nm_beam_topk_step_wide given statistics", k, lambda: _wide(s, k, True), s)
        record("nm_beam_topk_step_wide computed statistics", k, lambda: _wide(s, k, False), s)
        del s
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"B": B, "V": V, "hbm_peak_bytes_per_s": HBM_PEAK, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
