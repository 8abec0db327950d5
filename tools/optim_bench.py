"""HIP-event timings of the optimizers' clip + update launch (pass 3 of the flat optimizer) on the flat buffers of the
headline model -- bench.py's training configuration: vocabulary 32000, hidden 512; the element count is read from the
store -- for Adam (kind 0) and GradientDescent, Momentum, Adagrad, RMSProp (kinds 2..5), all instantiations of
csrc/nm_optim.hip's update kernel.

Per element an update moves 4-byte streams: Adam and RMSProp 7 (theta, both slots read and written; the gradient
read), Momentum and Adagrad 5, GradientDescent 3.  The table gives, per kind, the median microseconds per update, the
bytes moved over that time as a share of the 8 TB/s HBM peak (the buffers are several times the 256 MB Infinity Cache),
and the condition of the family: a new kind's median is at most Adam's median of the same call plus the spread (maximum
minus minimum) of Adam's own repeats.

Every repeat times ``--inner`` launches of one kind back to back between one pair of events; the kinds alternate within
a repeat, so drift of the machine falls on all of them alike.  Three untimed rounds come first.  The norms the clip
reads are computed once (nm_optim_regularize_norms); the learning rate is tiny, so the values stay where they are over
the thousands of updates of a run.

    python tools/optim_bench.py [--repeats 15] [--inner 20] [--out profiles/optim_family.md]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmonkey_amd import synthetic             # noqa: E402

HBM_PEAK = 8.0e12
# kind -> (name, streams of 4 bytes per element, slots, the four scalars)
KINDS = {0: ("Adam", 7, 2, (1e-7, 0.9, 0.999, 1e-8)),
         2: ("GradientDescent", 3, 0, (1e-7, 0.0, 0.0, 0.0)),
         3: ("Momentum", 5, 1, (1e-7, 0.9, 0.0, 0.0)),
         4: ("Adagrad", 5, 1, (1e-7, 0.0, 0.0, 0.0)),
         5: ("RMSProp", 7, 2, (1e-7, 0.9, 0.5, 1e-10))}


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--len", type=int, default=50, dest="length")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/optim_bench.py measures on a GPU; none is visible")
    dev = "cuda:0"
    h = args.hidden
    model = synthetic.build_translation_model(vocab_src=args.vocab, vocab_tgt=args.vocab, emb=h, rnn=h,
                                              max_len=args.length, beam_size=5, max_steps=args.length,
                                              length_normalization=0.6, l2_weight=1e-8, clip_norm=1.0,
                                              device=dev, seed=1234)
    store = model.tf_manager.sessions[0].store
    synthetic.load_baseline_weights(store, seed=1234, std=0.05)
    tables = model.trainer._optim_tables(store)                                # pylint: disable=protected-access
    gen = torch.Generator(device=dev).manual_seed(7)
    grad = torch.randn(store.total, device=dev, generator=gen) * 0.01
    # every kind owns its slots (Adam's signed first moment is no accumulator of squares: Adagrad would take the root of
    # a negative number); all of them start positive
    slots = {kind: [torch.rand(store.total, device=dev, generator=gen) * 0.1 + 0.1 for _ in range(spec[2])] + [None, None]
             for kind, spec in KINDS.items()}
    tables.regularize_and_norms(store.theta, grad, 0.0, 1e-8)
    trained = sum(store.specs[n].size for n in model.trainer.var_list(store))

    def launch(kind):
        tables.apply(kind, store.theta, grad, slots[kind][0], slots[kind][1], 1.0, KINDS[kind][3])

    def timed(kind):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            launch(kind)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.inner          # microseconds per update

    for _ in range(3):
        for kind in KINDS:
            timed(kind)
    times = {kind: [] for kind in KINDS}
    for _ in range(args.repeats):
        for kind in KINDS:                                   # the kinds alternate within a repeat
            times[kind].append(timed(kind))
    assert bool(torch.isfinite(store.theta).all())
    adam = times[0]
    adam_med, spread = median(adam), max(adam) - min(adam)
    rows, res = [], {"elements": int(store.total), "trained_elements": int(trained), "repeats": args.repeats,
                     "inner": args.inner, "adam_spread_us": round(spread, 2), "kinds": {}}
    for kind, (name, streams, _, _) in KINDS.items():
        med = median(times[kind])
        share = 4.0 * streams * trained / (med * 1e-6) / HBM_PEAK
        ok = None if kind == 0 else bool(med <= adam_med + spread)
        res["kinds"][name] = {"kind": kind, "us": round(med, 2), "min_us": round(min(times[kind]), 2),
                              "max_us": round(max(times[kind]), 2), "streams": streams,
                              "hbm_share": round(share, 4), "within_adam_plus_spread": ok}
        rows.append("| {} | {} | {} | {:.1f} | {:.1f} .. {:.1f} | {:.1f} % | {} |".format(
            kind, name, streams, med, min(times[kind]), max(times[kind]), 100 * share,
            "-" if ok is None else ("yes" if ok else "NO")))
    table = "\n".join(
        ["{} elements in the flat buffer, {} of them trained; {} repeats of {} back-to-back updates per kind, kinds "
         "alternating; Adam's repeats span {:.1f} us (maximum minus minimum).".format(
             store.total, trained, args.repeats, args.inner, spread), "",
         "| kind | optimizer | 4-byte streams | median us / update | min .. max | share of 8 TB/s HBM peak | "
         "<= Adam + spread |", "|---|---|---|---|---|---|---|"] + rows)
    print(table)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("# The optimizer family's update launch on the headline model's flat buffer\n\n"
                     "Written by `python tools/optim_bench.py --out {}` on an MI355X.\n\n".format(args.out))
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
