#!/usr/bin/env python
"""Benchmark of the attention-decoder hot path on MI355X (BASELINE.json metric).

One "step" = one optimizer step (forward + hand-written backward + clip + Adam)
of the translation.ini-shape model (biGRU-512 encoder, Bahdanau attention,
GRU-512 decoder, V=32000, weights of BASELINE.md section 3) on one synthetic batch
of B=128 sentences per GPU, src_len=tgt_len=50, driven through
``TensorFlowManager.execute`` exactly as the reference's training loop does.
``value`` = target tokens (non-pad target positions incl. </s>) per second over
all GPUs.  The timed loop rotates through 8 DISTINCT batches that are resident in
HBM when the timed region starts (never the same batch twice in a row).

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus 1 --steps 20 --warmup 3 --full
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times exactly --steps steps and prints ONE JSON line (rank 0): the headline
(``metric``, ``value``, ``unit``, ``higher_is_better``, ``dtype``, ``ms_per_step``), the workload, the loss of the
last step, the data-parallel exchange (N > 1) and ``roofline_train`` (the timed step against the fp32 matrix peak,
from the same timing).  ``--dump-outputs DIR`` writes what the last timed step returned, its losses, as
DIR/<name>.npy (``dump_outputs``).

``--full`` adds to the same line, measured after the headline's timed steps:
  ``beam5_*``, ``greedy_*``  beam-5 and greedy decoding of the headline model;
  ``ms_per_step_fresh``, ``ms_per_step_strings``  the timed loop with batches assembled on the host and uploaded
                     inside the step (pre-indexed int32 ids; token strings, the reference's feeding model);
  ``other_scaling``  the strong split next to the weak one (N > 1);
  ``roofline``       the fused Bahdanau attention step (nm_attn_fwd = ONE launch of attn_whole_fast<13>:
                     score + softmax + mask-renorm + context of a decoding step), HBM-bound, timed live
                     with HIP events on its stream: ``achieved`` / ``frac`` = 32 back-to-back launches
                     over 8 key / value sets that evict each other (cold, one event pair around the
                     sequence); ``achieved_warm`` inside a greedy decode (keys sit in the 256 MB Infinity
                     Cache between steps), ``achieved_cold_single`` one launch behind a 1 GB sweep;
                     ``traffic`` and ``rocprof_kernel_us`` from the newest committed rocprofv3 passes of
                     the same kernel (tools/attn_evidence.sh -> profiles/rNN_attn_step_*.json);
  ``roofline_step``  the whole greedy decoder step against its ~165 MB of algorithmic traffic;
  ``cpu_baseline``   torch-CPU / NumPy restatement of the reference's step (NOT TF 1.12 -- TF cannot
                     be installed here) on the headline batch (B=128): SURVEY 8(d)'s protocol (8 threads,
                     median of 5 after 2 warm-ups) on a bounded sample, next to it all host threads;
  ``configs``        BASELINE configs[3] (captioning) and configs[4] (Transformer-base) at their own shapes, the taped
                     general path (NematusGRU + conditional GRU) at the headline size:
                     training step, greedy and beam-5 decoding, each with its own roofline.
"""
import argparse
import ctypes
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0        # MI355X HBM3E spec (MI355X_MICROARCH.md)
MFMA_F32_PEAK_TF = 157.3      # fp32 matrix peak (v_mfma_f32_32x32x2_f32), same guide
NUM_BATCHES = 8               # distinct batches rotated through the timed loop


def newest_profile(pattern):
    """Newest round's committed evidence file matching ``profiles/<pattern>`` (rNN_ prefixes sort by round)."""
    import glob
    hits = sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)))
    return hits[-1] if hits else None


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128, help="sentences per GPU (weak scaling)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak: --batch sentences per GPU (default, what the driver runs); strong: --batch "
                         "sentences per optimizer step in total, sharded over the GPUs (BASELINE.json's "
                         "'shards minibatches': 16 per GPU at N=8)")
    ap.add_argument("--len", type=int, default=50, dest="length")
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--beam-batches", type=int, default=4, help="beam-5 decode batches to time (0 = skip)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-batch", type=int, default=128, help="sentences of the CPU baseline's training sample")
    ap.add_argument("--cpu-steps", type=int, default=2, help="timed full-batch CPU training steps on all threads "
                                                             "(after 1 warm-up)")
    ap.add_argument("--cpu-sample", type=int, default=16, help="sentences of the 8-thread CPU baseline's sample")
    ap.add_argument("--cpu-beam-batch", type=int, default=16, help="sentences of the CPU baseline's beam-5 sample")
    ap.add_argument("--no-feed-legs", action="store_true", help="skip the fresh / strings feeding legs")
    ap.add_argument("--no-configs", action="store_true",
                    help="skip the legs of BASELINE configs[3] (captioning) and configs[4] (Transformer)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure decoding, the host-fed step, the attention roofline, the "
                         "other configurations and the CPU baseline (the options above shape these legs)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step returned (its losses) as DIR/<name>.npy")
    return ap.parse_args()


def attention_step_bytes(b, s, a, c):
    """Algorithmic bytes of one fused attention step."""
    return 4 * (b * s * a + b * s * c + 2 * b * s + b * a + b * c)


def decoder_step_bytes(b, s, h, v):
    """Algorithmic bytes of one greedy decoder step as SURVEY 8d defines them (~165 MB at the headline
    shape): attention stream 53.5 + GRU kernels 6.3 + query projection 2.1 + output projection 4.2 +
    vocabulary projection 65.5 + logits written 16.4 + logits read back for the argmax 16.4 (MB).  The
    definition is kept as published even where a fused epilogue no longer re-reads the logits."""
    e, c, a = h, 2 * h, 2 * h
    weights = 4 * ((e + h) * 3 * h + h * a + (h + e + c) * e + e * v + v)
    return attention_step_bytes(b, s, a, c) + weights + 2 * 4 * b * v


def cpu_baseline(args):
    """The reference's step restated for the host CPU at the reference's op granularity (per-step cell /
    attention / projection / logits): training = oracle/torch_ref.py (torch-CPU fp32, autograd), beam-5 =
    oracle/nm_oracle.py (NumPy).  NOT TensorFlow 1.12 (cannot be installed here).

    Primary figure = SURVEY 8(d)'s protocol: ``torch.set_num_threads(8)``, median of 5 optimizer steps after 2
    warm-ups, on a BOUNDED SAMPLE of the headline workload -- ``--cpu-sample`` (16) of the batch's 128 sentences, all
    lengths 50, V and H as timed on the GPU (the full batch takes ~15 s per step on the host: seven of them would
    not fit the few minutes a default run may take).  Next to it (``all_threads``): the full headline batch on every
    host thread, median of ``--cpu-steps`` after 1 warm-up -- faster per token, but it wanders with whatever else
    the host is doing.  Beam-5: ``--cpu-beam-batch`` sentences x 50 steps, NumPy, one pass."""
    from oracle import nm_oracle as O
    from oracle import torch_ref as TR
    h = args.hidden
    params = O.init_params(seed=1234, vocab_src=args.vocab, vocab_tgt=args.vocab, emb=h, rnn=h)
    src, tgt_tb = O.synthetic_batch(seed=1234, batch=args.cpu_batch, src_len=args.length, tgt_len=args.length,
                                    vocab=args.vocab, ragged=False)

    def steps(bsz, warm, timed):
        tp = TR.to_torch(params)
        m = {k: torch.zeros_like(v) for k, v in tp.items()}
        v = {k: torch.zeros_like(x) for k, x in tp.items()}
        times = []
        for step in range(1, warm + timed + 1):
            t0 = time.perf_counter()
            _, _, _, grads = TR.train_step_grads(tp, src[:bsz], tgt_tb[:, :bsz], l1_weight=0.0, l2_weight=1e-8)
            TR.clip_and_adam(tp, grads, m, v, step, 1.0)
            times.append(time.perf_counter() - t0)
        return float(np.median(times[warm:]))
    all_threads = torch.get_num_threads()
    sample = max(1, min(args.cpu_batch, args.cpu_sample))
    torch.set_num_threads(8)
    try:
        sec8 = steps(sample, 2, 5)
    finally:
        torch.set_num_threads(all_threads)
    sec_all = steps(args.cpu_batch, 1, args.cpu_steps)
    # beam-5 over the full 50 steps (</s> unreachable, as in the GPU leg)
    bb = max(1, min(args.cpu_batch, args.cpu_beam_batch))
    pb = dict(params)
    bias = pb["decoder/state_to_word_b"].copy()
    bias[O.END] = -1e9
    pb["decoder/state_to_word_b"] = bias
    enc = O.sentence_encoder(pb, src[:bb])
    t0 = time.perf_counter()
    O.beam_search(pb, O.DecoderSpec(max_output_len=args.length), enc, 5, args.length, 0.6)
    beam_sec = time.perf_counter() - t0
    return {"value": sample * args.length / sec8, "unit": "tokens/s", "cores": 8, "kind": "port",
            "sample": "training: {} of the headline batch's 128 sentences x len {} (ragged=False as on the GPU), V={} "
                      "H={}, torch.set_num_threads(8), median of 5 optimizer steps after 2 warm-ups (SURVEY 8d), "
                      "torch-CPU fp32 restatement of the reference step, not TF 1.12; beam-5: {} sentences x {} steps, "
                      "NumPy restatement, one pass".format(sample, args.length, args.vocab, h, bb, args.length),
            "sec_per_step": sec8,
            "all_threads": {"value": args.cpu_batch * args.length / sec_all, "unit": "tokens/s", "cores": all_threads,
                            "sample": "the full headline batch, B={}, median of {} steps after 1 warm-up".format(
                                args.cpu_batch, args.cpu_steps), "sec_per_step": sec_all},
            "beam5_tok_s": bb * args.length / beam_sec, "beam5_sec": beam_sec}


def _timed_gpu(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def transformer_leg(args, dev):
    """BASELINE configs[4]: Transformer-base (6 + 6 layers, d=512, 8 heads, ff 2048, tied embeddings), B=128,
    len 50, V=32000, beam 5 -- training step, greedy and beam-5 decoding through the key/value cache."""
    from neuralmonkey_amd import synthetic
    batch, length, vocab = args.batch, args.length, args.vocab
    m = synthetic.build_transformer_model(vocab=vocab, max_len=length, max_steps=length, device=dev, seed=1234)
    tfm = m.tf_manager
    store = tfm.sessions[0].store
    synthetic.load_baseline_weights(store, seed=1234, std=0.05)
    pool = [synthetic.synthetic_dataset(seed=4000 + i, batch=batch, src_len=length, tgt_len=length, vocab=vocab)
            for i in range(4)]
    it = iter(range(1 << 30))
    res = {}

    def train():
        res["out"] = tfm.execute(pool[next(it) % 4], m.trainer.feedables, [m.trainer], train=True)[0]
    t_train = _timed_gpu(train, 3, 8)
    tokens = batch * length
    flops = synthetic.transformer_train_flops(batch, length, vocab)
    # decode the full length: with tied embeddings (W = E^T, no bias) </s> cannot be pushed down by a bias, so the
    # final layer norm gets a large offset along one direction and the </s> embedding points the other way
    u = torch.zeros(store["decoder/LayerNorm/beta"].shape[0], device=dev)
    u[0] = 1.0
    store["decoder/LayerNorm/beta"].copy_(10.0 * u)
    store["decoder/word_embeddings"][2].copy_(-100.0 * u)
    dsd = [synthetic.synthetic_dataset(seed=5000 + i, batch=batch, src_len=length, tgt_len=length, vocab=vocab,
                                       with_target=False) for i in range(2)]
    out = {}
    for name, runner in (("greedy", m.greedy_runner), ("beam5", m.beam_runner)):
        t = _timed_gpu(lambda: tfm.execute(dsd[next(it) % 2], runner.feedables, [runner], compute_losses=False), 2, 3)
        r = tfm.execute(dsd[0], runner.feedables, [runner], compute_losses=False)[0]
        steps = max(len(sent) for sent in r.outputs[runner.output_series])
        out[name] = (t, steps)
    tf = flops / t_train / 1e12
    # one cached decoding step against the fp32 matrix peak: how far the launch chain of a step is from its products
    dec_flops = {name: synthetic.transformer_decode_step_flops(batch * (5 if name == "beam5" else 1), vocab,
                                                               cached_len=length // 2, src_len=length)
                 for name in ("greedy", "beam5")}
    roofline_decode = {}
    for name in ("greedy", "beam5"):
        us = out[name][0] / max(1, out[name][1]) * 1e6
        ach = dec_flops[name] / (us * 1e-6) / 1e12
        roofline_decode[name] = {"bound": "mfma", "rows": batch * (5 if name == "beam5" else 1), "us_per_step": us,
                                 "flops_per_step": dec_flops[name], "achieved": ach, "peak": MFMA_F32_PEAK_TF,
                                 "unit": "TFLOP/s", "frac": ach / MFMA_F32_PEAK_TF}
    roofline_decode["what"] = ("one cached decoding step (mean over the steps of a batch): 2 x multiply-adds of the six "
                               "decoder layers' projections, both attention cores (own prefix at half the length, "
                               "encoder at full length), the feed-forward blocks and the tied vocabulary projection "
                               "(synthetic.transformer_decode_step_flops); a step is a chain of ~70 dependent launches "
                               "of 128- or 640-row products: launch-latency-bound, not matrix-bound "
                               "(profiles/r06_transformer_{greedy,beam}_kernel_stats.csv)")
    return {"workload": "tests/transformer.ini-shape at the Transformer-base size: 6+6 layers, d=512, 8 heads, ff 2048, "
                        "tied embeddings, B={}, len={}, V={}, CrossEntropyTrainer(l2=1e-8, clip_norm=1.0) + Adam, "
                        "weights N(0,0.05), 4 HBM-resident batches in rotation".format(batch, length, vocab),
            "parameters": int(store.total), "train_ms_per_step": t_train * 1e3, "train_tok_s": tokens / t_train,
            "loss": res["out"].losses["decoder - cost"],
            "greedy_ms_per_batch": out["greedy"][0] * 1e3, "greedy_steps": out["greedy"][1],
            "greedy_tok_s": batch * out["greedy"][1] / out["greedy"][0],
            "beam5_ms_per_batch": out["beam5"][0] * 1e3, "beam5_steps": out["beam5"][1],
            "beam5_tok_s": batch * out["beam5"][1] / out["beam5"][0],
            "roofline": {"bound": "mfma", "what": "whole training step: 2 x multiply-adds of every dense product, "
                                                  "forward + backward (synthetic.transformer_train_flops)",
                         "flops_per_step": flops, "achieved": tf, "peak": MFMA_F32_PEAK_TF, "unit": "TFLOP/s",
                         "frac": tf / MFMA_F32_PEAK_TF},
            "roofline_decode": roofline_decode}


def general_path_leg(args, dev):
    """The TAPED general path at the headline size (no BASELINE config of its own: what tests/small.ini = configs[0] and
    every Nematus-style experiment run on): NematusGRU bidirectional encoder + Bahdanau attention + conditional
    NematusGRU decoder (nn/ortho_gru_cell.py:57-105, decoders/decoder.py:303-325), H = E = 512, B = 128, len 50,
    V = 32000.  The encoder layer's time loops are one cluster launch each way (nm_nematus_seq_fwd / _bwd); the
    conditional decoder steps launch by launch inside one HIP graph per batch shape."""
    from neuralmonkey_amd import synthetic
    from neuralmonkey_amd.attention import Attention
    from neuralmonkey_amd.decoders import BeamSearchDecoder, Decoder
    from neuralmonkey_amd.encoders import SentenceEncoder
    from neuralmonkey_amd.runners import BeamSearchRunner, GreedyRunner
    from neuralmonkey_amd.runtime import reset_registry
    from neuralmonkey_amd.tf_manager import TensorFlowManager
    from neuralmonkey_amd.trainers import CrossEntropyTrainer
    batch, length, vocab, h = args.batch, args.length, args.vocab, args.hidden
    reset_registry()
    sv, tv = synthetic.synthetic_vocabulary(vocab), synthetic.synthetic_vocabulary(vocab)
    cell = os.environ.get("NM_GP_CELL", "NematusGRU")          # (tools/general_path_probe.py: LSTM layers and decoder)
    enc = SentenceEncoder(name="encoder", vocabulary=sv, data_id="source", embedding_size=h, rnn_size=h,
                          max_input_len=length, rnn_cell=cell)
    att = Attention(name="attention", encoder=enc)
    dec = Decoder(encoders=[enc], vocabulary=tv, data_id="target", name="decoder", max_output_len=length,
                  embedding_size=h, rnn_size=h, attentions=[att], rnn_cell=cell, conditional_gru=cell != "LSTM")
    bdec = BeamSearchDecoder(name="beam_decoder", parent_decoder=dec, beam_size=5, max_steps=length,
                             length_normalization=0.6)
    greedy, beam = GreedyRunner(output_series="target", decoder=dec), BeamSearchRunner(output_series="target_beam",
                                                                                      decoder=bdec, rank=1)
    trainer = CrossEntropyTrainer(decoders=[dec], l2_weight=1e-8, clip_norm=1.0)
    tfm = TensorFlowManager(num_sessions=1, num_threads=4, device=dev, seed=1234)
    tfm.initialize_sessions()
    store = tfm.sessions[0].store
    synthetic.load_baseline_weights(store, seed=1234, std=0.05)
    pool = [synthetic.synthetic_dataset(seed=8000 + i, batch=batch, src_len=length, tgt_len=length, vocab=vocab)
            for i in range(2)]
    it = iter(range(1 << 30))
    res = {}

    def train():
        res["out"] = tfm.execute(pool[next(it) % 2], trainer.feedables, [trainer], train=True)[0]
    t_train = _timed_gpu(train, 3, 6)
    if getattr(args, "general_train_only", False):              # (tools/general_path_probe.py --train-only, for profiles)
        return {"train_ms_per_step": t_train * 1e3, "loss": res["out"].losses["decoder - cost"]}
    store["decoder/state_to_word_b"][2] = -1e9                   # </s> unreachable: all steps run
    dsd = [synthetic.synthetic_dataset(seed=9000 + i, batch=batch, src_len=length, tgt_len=length, vocab=vocab,
                                       with_target=False) for i in range(2)]
    out = {}
    for name, runner in (("greedy", greedy), ("beam5", beam)):
        t = _timed_gpu(lambda: tfm.execute(dsd[next(it) % 2], runner.feedables, [runner], compute_losses=False), 2, 3)
        r = tfm.execute(dsd[0], runner.feedables, [runner], compute_losses=False)[0]
        out[name] = (t, max(len(sent) for sent in r.outputs[runner.output_series]))
    tokens = batch * length
    return {"workload": "general (taped) path: NematusGRU biRNN encoder + Bahdanau attention + conditional NematusGRU "
                        "decoder, H=E={}, B={}, len={}, V={}, CrossEntropyTrainer + Adam".format(h, batch, length, vocab),
            "train_ms_per_step": t_train * 1e3, "train_tok_s": tokens / t_train,
            "loss": res["out"].losses["decoder - cost"],
            "greedy_ms_per_batch": out["greedy"][0] * 1e3, "greedy_steps": out["greedy"][1],
            "beam5_ms_per_batch": out["beam5"][0] * 1e3, "beam5_steps": out["beam5"][1]}


def captioning_leg(args, dev, lib):
    """BASELINE configs[3]: pre-extracted 8x8x2048 maps -> SpatialFiller -> Bahdanau attention over the 64 positions
    (state 512) -> GRU-512 decoder, B=128, target len 50, V=32000, beam 5."""
    from neuralmonkey_amd import synthetic
    batch, length, vocab, shape, asz = args.batch, args.length, args.vocab, (8, 8, 2048), 512
    m = synthetic.build_captioning_model(vocab=vocab, shape=shape, att_size=asz, max_len=length, max_steps=length,
                                         device=dev, seed=1234)
    tfm = m.tf_manager
    store = tfm.sessions[0].store
    synthetic.load_baseline_weights(store, seed=1234, std=0.05)
    pool = [synthetic.synthetic_captioning_dataset(seed=6000 + i, batch=batch, shape=shape, tgt_len=length, vocab=vocab)
            for i in range(2)]
    it = iter(range(1 << 30))
    res = {}

    def train():
        res["out"] = tfm.execute(pool[next(it) % 2], m.trainer.feedables, [m.trainer], train=True)[0]
    t_train = _timed_gpu(train, 3, 8)
    store["decoder/state_to_word_b"][2] = -1e9                   # </s> unreachable: all 50 steps run
    dsd = [synthetic.synthetic_captioning_dataset(seed=7000 + i, batch=batch, shape=shape, tgt_len=length, vocab=vocab,
                                                  with_target=False) for i in range(2)]
    out = {}
    for name, runner in (("greedy", m.greedy_runner), ("beam5", m.beam_runner)):
        t = _timed_gpu(lambda: tfm.execute(dsd[next(it) % 2], runner.feedables, [runner], compute_losses=False), 2, 3)
        r = tfm.execute(dsd[0], runner.feedables, [runner], compute_losses=False)[0]
        steps = max(len(sent) for sent in r.outputs[runner.output_series])
        out[name] = (t, steps)
    # the attention step kernel at this shape (one query per image, 64 positions x 2048 channels), warm, inside an
    # eagerly launched greedy decode with HIP events around every nm_attn_fwd call
    sess0 = tfm.sessions[0]
    graphs_were = sess0.use_graphs
    sess0.use_graphs = False
    lib.nm_prof_enable(None, 1)
    tfm.execute(dsd[0], m.greedy_runner.feedables, [m.greedy_runner], compute_losses=False)
    torch.cuda.synchronize()
    lib.nm_prof_enable(None, 0)
    sess0.use_graphs = graphs_were
    tot_ms, cnt = ctypes.c_double(0.0), ctypes.c_int64(0)
    lib.nm_prof_attn_step(None, ctypes.byref(tot_ms), ctypes.byref(cnt))
    s, c = shape[0] * shape[1], shape[2]
    nbytes = attention_step_bytes(batch, s, asz, c)
    att_us = (tot_ms.value * 1e3 / cnt.value) if cnt.value else None
    warm_gbps = (nbytes / (att_us * 1e-6) / 1e9) if att_us else None
    # COLD: launches back to back over NSETS distinct key / value sets (4 x 84 MB > the 256 MB Infinity Cache: a set
    # is evicted before its next visit), one event pair around the sequence -- the protocol of the headline figure
    from neuralmonkey_amd import ops
    gen = torch.Generator(device=dev).manual_seed(7)
    NSETS, ROUNDS = 4, 6
    sets = [(torch.randn(batch, s, asz, device=dev, generator=gen), torch.randn(batch, s, c, device=dev, generator=gen))
            for _ in range(NSETS)]
    y = torch.randn(batch, asz, device=dev, generator=gen)
    vv = torch.randn(asz, device=dev, generator=gen)
    mask, bias = torch.ones(batch, s, device=dev), torch.zeros(1, device=dev)
    ctx_o, wts = torch.empty(batch, c, device=dev), torch.empty(batch, s, device=dev)
    ws = ops.attn_workspace(batch, s, c, dev)

    def rotate(rounds):
        for i in range(rounds * NSETS):
            ops.attn_fwd(y, sets[i % NSETS][0], sets[i % NSETS][1], mask, vv, bias, 1, ctx_o, wts, ws)
    rotate(1)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    rotate(ROUNDS)
    ev1.record()
    torch.cuda.synchronize()
    cold_us = ev0.elapsed_time(ev1) * 1e3 / (ROUNDS * NSETS)
    cold_gbps = nbytes / (cold_us * 1e-6) / 1e9
    del sets
    traffic, rocprof_us, files = None, {}, []
    pmc = newest_profile("r[0-9][0-9]_attn_cap_pmc_cold.json")
    if pmc:
        with open(pmc) as fh:
            traffic = json.load(fh).get("hbm_bytes_per_launch")
        files.append(os.path.relpath(pmc, ROOT))
    for mode in ("cold", "warm", "dirty"):
        path = newest_profile("r[0-9][0-9]_attn_cap_trace_{}.json".format(mode))
        if path:
            with open(path) as fh:
                rocprof_us[mode] = json.load(fh).get("sum_avg_us")
            files.append(os.path.relpath(path, ROOT))
    tokens = batch * length
    return {"workload": "tests/captioning.ini-shape: 8x8x2048 maps (N(0,1) clipped at 0) -> SpatialFiller -> Attention("
                        "state {}) -> GRU-512 decoder, B={}, target len={}, V={}, CrossEntropyTrainer + Adam".format(
                            asz, batch, length, vocab),
            "train_ms_per_step": t_train * 1e3, "train_tok_s": tokens / t_train,
            "loss": res["out"].losses["decoder - cost"],
            "greedy_ms_per_batch": out["greedy"][0] * 1e3, "greedy_steps": out["greedy"][1],
            "greedy_tok_s": batch * out["greedy"][1] / out["greedy"][0],
            "beam5_ms_per_batch": out["beam5"][0] * 1e3, "beam5_steps": out["beam5"][1],
            "beam5_tok_s": batch * out["beam5"][1] / out["beam5"][0],
            "roofline": {"bound": "hbm", "kernel": "nm_attn_fwd at S=64, A={}, C=2048 (one decoding step)".format(asz),
                         "timing": "COLD: {} back-to-back launches over {} key / value sets that evict each other "
                                   "(one HIP event pair on the launch stream around the sequence); achieved_warm: "
                                   "inside a greedy decode (the maps stay in the Infinity Cache between steps), event "
                                   "pairs around single calls (event-pair cost included)".format(ROUNDS * NSETS, NSETS),
                         "algorithmic_bytes_per_launch": nbytes, "launch_us": cold_us, "launches": ROUNDS * NSETS,
                         "achieved": cold_gbps, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": cold_gbps / HBM_PEAK_GBPS,
                         "achieved_warm": warm_gbps, "launch_us_warm": att_us,
                         "traffic": traffic, "rocprof_kernel_us": rocprof_us or None,
                         "evidence": files or None}}


def time_loops_leg(args, dev):
    """The four GRU time loops of the headline training step on their own (rows = --batch, H = --hidden, --len steps):
    microseconds per recurrent step, HIP-graph replayed, as ONE cluster launch per loop (csrc/nm_gru_cluster.hip --
    what the timed training step runs) and as two launches per step (the round-4 path, NM_CLUSTER_LOOPS=0)."""
    from neuralmonkey_amd import ops
    from neuralmonkey_amd.nn import gru
    rows, h, s = args.batch, args.hidden, args.length
    g = torch.Generator(device=dev).manual_seed(0)
    out = {}
    for ndir, tag in ((1, "decoder"), (2, "encoder_2dir")):
        rn = lambda *shape: torch.randn(*shape, device=dev, generator=g) * 0.1
        xp, wgh, wch = rn(rows * s, ndir * 3 * h), rn(ndir, h, 2 * h), rn(ndir, h, h)
        hcur, states = torch.zeros(ndir, rows, h, device=dev), torch.zeros(rows, s, ndir * h, device=dev)
        ru_all, c_all = torch.empty(s, ndir, rows, 2 * h, device=dev), torch.empty(s, ndir, rows, h, device=dev)
        rh = torch.empty(ndir, rows, h, device=dev)
        dh, d_out = torch.zeros(ndir, rows, h, device=dev), rn(rows, s, ndir * h)
        dxp = torch.zeros(rows * s, ndir * 3 * h, device=dev)
        scratch = (torch.empty(2, ndir, rows, 2 * h, device=dev), torch.empty(ndir, rows, h, device=dev),
                   torch.empty(ndir, rows, h, device=dev))
        xst, seq = (3 * h, s * ndir * 3 * h, ndir * 3 * h), (h, s * ndir * h, ndir * h)

        def fwd_steps():
            hcur.zero_()
            for t in range(s):
                gru.step_fwd(xp, xst, hcur, hcur, wgh, wch, ru_all[t], rh, c_all[t], states, seq, None, t, ndir, rows, h,
                             False, None, None)

        def bwd_steps():
            dh.zero_()
            gru.bptt(s, dh, d_out, seq, ru_all, c_all, None, states, seq, dxp, xst, wgh, wch, None, ndir, rows, h, False,
                     *scratch)

        def replayed(fn, reps=10):
            fn()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                fn()
            graph.replay()
            return _timed_gpu(graph.replay, 1, reps) * 1e6 / s
        entry = {"two_launches_per_step": {"forward_us_per_step": replayed(fwd_steps), "bptt_us_per_step": replayed(bwd_steps)}}
        if ops.gru_seq_supported(rows, h, ndir):
            ws = ops.gru_seq_workspace(rows, h, ndir, dev)

            def fwd_cluster():
                hcur.zero_()
                ops.gru_seq_fwd(s, ndir, rows, h, xp, xst, hcur, hcur, 0, ru_all[0], ndir * rows * 2 * h, None, 0,
                                c_all[0], ndir * rows * h, wgh, wch, ws, out=states, out_strides=seq)

            def bwd_cluster():
                dh.zero_()
                ops.gru_seq_bwd(s, ndir, rows, h, dh, d_out, seq, ru_all[0], ndir * rows * 2 * h, c_all[0], ndir * rows * h,
                                None, states, seq, dxp, xst, wgh, wch, ws)
            entry["one_cluster_launch_per_loop"] = {"forward_us_per_step": replayed(fwd_cluster),
                                                    "bptt_us_per_step": replayed(bwd_cluster),
                                                    "gave_up": bool(ops.gru_seq_failed(ws))}
        out[tag] = entry
    return {"what": "GRU time loops alone, us per recurrent step ({} rows, H = {}, {} steps, HIP-graph replayed)".format(
        rows, h, s), "dtype": "f32", **out}


def split_projection_leg(args, dev):
    """OPT-IN (NM_PROJ_SPLIT=1), its own dtype, NOT the number of record: greedy and beam-5 decoding of the headline
    model with the steps' vocabulary projection on the bf16 matrix cores -- operands split three ways into bf16 (24
    mantissa bits), six products, fp32 accumulate (csrc/nm_gemm_bf16x3.hip gemm_split6_stats) -- next to the
    exact-fp32 projection every number above uses.  A model of its own (fresh decoding graphs), the same weights and
    batches as the main decoding legs; the accuracy of the product against float64 beside the exact kernel's."""
    from neuralmonkey_amd import ops, synthetic
    h = args.hidden
    ops.PROJ_SPLIT = True
    try:
        model = synthetic.build_translation_model(vocab_src=args.vocab, vocab_tgt=args.vocab, emb=h, rnn=h,
                                                  max_len=args.length, beam_size=5, max_steps=args.length,
                                                  length_normalization=0.6, with_trainer=False, device=dev, seed=1234)
        tfm = model.tf_manager
        store = tfm.sessions[0].store
        synthetic.load_baseline_weights(store, seed=1234, std=0.05)
        store["decoder/state_to_word_b"][2] = -1e9                 # </s> unreachable: all steps run
        dsd = [synthetic.synthetic_dataset(seed=99 + 10 * i, batch=args.batch, src_len=args.length, tgt_len=args.length,
                                           vocab=args.vocab, with_target=False) for i in range(4)]
        out = {}
        for name, runner in (("greedy", model.greedy_runner), ("beam5", model.beam_runner)):
            for i in range(5):
                tfm.execute(dsd[i % 4], runner.feedables, [runner], compute_losses=False, lookahead=dsd[(i + 1) % 4])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 6
            for i in range(n):
                tfm.execute(dsd[i % 4], runner.feedables, [runner], compute_losses=False,
                            lookahead=dsd[(i + 1) % 4] if i + 1 < n else None)
            torch.cuda.synchronize()
            out[name] = (time.perf_counter() - t0) / n
        # the product itself at the two decoding shapes: time per launch and error against float64, both kernels
        w, bias = store["decoder/state_to_word_W"], store["decoder/state_to_word_b"].clone()
        bias[2] = 0.0                                              # (the -1e9 above would be the error's yardstick)
        gen = torch.Generator(device=dev).manual_seed(5)
        product = {}
        for rows in (args.batch, 5 * args.batch):
            a = torch.randn(rows, h, device=dev, generator=gen)
            want = a.double() @ w.double() + bias.double()
            st, lg = ops.logits_stats_buffer(rows, args.vocab, dev), torch.empty(rows, args.vocab, device=dev)
            planes = ops.proj_split_prepare(w)
            t3 = _timed_gpu(lambda: ops.logits_stats_gemm(a, w, bias, st, out=lg), 3, 20) * 1e6
            e3 = float((lg.double() - want).abs().max() / want.abs().max())
            ops.proj_split_forget(w)
            t32 = _timed_gpu(lambda: ops.logits_stats_gemm(a, w, bias, st, out=lg), 3, 20) * 1e6
            e32 = float((lg.double() - want).abs().max() / want.abs().max())
            del planes
            product["rows_{}".format(rows)] = {"split_us": t3, "exact_f32_us": t32, "split_max_error_vs_float64": e3,
                                               "exact_f32_max_error_vs_float64": e32}
        tok = args.batch * args.length
        return {"dtype": "bf16x6 (fp32 operands split into bf16 hi + mid + lo: 24 mantissa bits; six bf16 MFMA products, "
                         "fp32 accumulate) for the vocabulary projection of the decoding steps; everything else f32",
                "switch": "NM_PROJ_SPLIT=1 (off by default: the exact-fp32 projection is the number of record)",
                "greedy_ms_per_batch": out["greedy"] * 1e3, "greedy_tok_s": tok / out["greedy"],
                "beam5_ms_per_batch": out["beam5"] * 1e3, "beam5_tok_s": tok / out["beam5"],
                "projection": product,
                "parity": "tests/test_proj_split_gpu.py: product error <= 2x the exact kernel's against float64, its "
                          "statistics exact for its own logits, and the decoding parity tests (full-size greedy / "
                          "beam accounting, the reference-executed fixtures) pass under the switch"}
    finally:
        ops.PROJ_SPLIT = False
        ops.proj_split_forget()


def bf16x3_costing_leg(args, dev, lib):
    """VERDICT r3 item 10 -- COSTED, NOT SHIPPED: the vocabulary projection's product shape (states . E^T, the tied /
    "NT" form: M = B*len, N = V, K = hidden) through a three-term split-bf16 emulation on the bf16 matrix cores
    (csrc/nm_gemm_bf16x3.hip) next to the exact-fp32 kernel every number above uses.  Its own dtype, its own entry;
    nothing in the headline or in the other configs runs it."""
    from neuralmonkey_amd import _lib, ops
    m, n, k = args.batch * args.length, args.vocab, args.hidden
    gen = torch.Generator(device=dev).manual_seed(3)
    a = torch.randn(m, k, device=dev, generator=gen)
    b = torch.randn(n, k, device=dev, generator=gen) * 0.05
    c32, c3 = torch.empty(m, n, device=dev), torch.empty(m, n, device=dev)

    def timed(fn, reps=10):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3
    t32 = timed(lambda: ops.gemm(a, b, out=c32, trans_b=True))
    call = lambda: _lib.check(lib.nm_gemm_bf16x3_nt(ops._stream(), m, n, k, a.data_ptr(), a.stride(0), b.data_ptr(),
                                                    b.stride(0), c3.data_ptr(), c3.stride(0), 3, 2), "nm_gemm_bf16x3_nt")
    t3 = timed(call)
    exact = a[:256].double() @ b.double().t()
    scale = float(exact.abs().max())
    flops = 2.0 * m * n * k
    return {"workload": "ONE product of the vocabulary-projection shape, C[{},{}] = A[{},{}] . B[{},{}]^T; costing only "
                        "(VERDICT r3 item 10): not used by any other number in this line".format(m, n, m, k, n, k),
            "dtype": "bf16x3 (fp32 operands split into bf16 hi + lo, three bf16 MFMA products, fp32 accumulate)",
            "us": t3, "tflops_equivalent": flops / t3 / 1e6,
            "max_error_vs_float64_rel_to_max": float((c3[:256].double() - exact).abs().max()) / scale,
            "exact_f32": {"dtype": "f32", "us": t32, "tflops": flops / t32 / 1e6,
                          "max_error_vs_float64_rel_to_max": float((c32[:256].double() - exact).abs().max()) / scale},
            "speedup_over_exact_f32": t32 / t3}


def dump_outputs(path, res):
    """What a caller of the timed training step receives from its last call (``TensorFlowManager.execute``'s
    ExecutionResult: a trainer returns its losses and no output series): one float64 file per loss, named after it.
    The variables and their gradients are the step's state, not its result; they are not written."""
    os.makedirs(path, exist_ok=True)
    for name, value in res.losses.items():
        np.save(os.path.join(path, "loss.{}.npy".format(re.sub(r"[^A-Za-z0-9_.-]+", "_", name))),
                np.array([value], dtype=np.float64))


def full_legs(args, dp, rank, world, dev, lib, model, tfm, pool, uploader, step, timed, fresh, barrier):
    """What ``--full`` measures after the headline's timed steps (module docstring); returns the fields it adds to
    rank 0's line (None on the other ranks, which take part in the collectives of the data-parallel legs)."""
    from neuralmonkey_amd import _lib, ops, synthetic
    from neuralmonkey_amd.dataset import Dataset
    h = args.hidden
    tokens_local = args.batch * args.length
    store = tfm.sessions[0].store

    # ---- beam-5 decode throughput (emitted rank-1 tokens up to and incl. </s>)
    beam_tok_s = beam_ms_per_batch = beam_b1_ms = None
    logit_b = store["decoder/state_to_word_b"]
    if args.beam_batches > 0:
        runner = model.beam_runner
        # synthetic decode workload: </s> is made unreachable so that every hypothesis runs the
        # full max_steps=len steps (6400 emitted rank-1 tokens per 128-sentence batch)
        saved_end_bias = float(logit_b[2].item())
        logit_b[2] = -1e9
        dsb = [synthetic.synthetic_dataset(seed=99 + 10 * i + rank, batch=args.batch, src_len=args.length,
                                           tgt_len=args.length, vocab=args.vocab, with_target=False)
               for i in range(min(4, args.beam_batches))]
        for i in range(5):                  # warm-up: eager pass (allocations) + HIP-graph capture pass, in BOTH
            #                                     buffer slots consecutive batches alternate between (look-ahead)
            out = tfm.execute(dsb[i % len(dsb)], runner.feedables, [runner], compute_losses=False,
                              lookahead=dsb[(i + 1) % len(dsb)])[0]
        barrier()
        tb = time.perf_counter()
        emitted = 0
        for i in range(args.beam_batches):
            # a stream of batches: the next batch's encoder runs on a second stream under this batch's search
            nxt = dsb[(i + 1) % len(dsb)] if i + 1 < args.beam_batches else None
            out = tfm.execute(dsb[i % len(dsb)], runner.feedables, [runner], compute_losses=False, lookahead=nxt)[0]
            emitted += sum(min(len(s) + 1, args.length) for s in out.outputs[runner.output_series])
        barrier()
        tb = time.perf_counter() - tb
        if dp:
            t = torch.tensor([tb, float(emitted)], dtype=torch.float64, device=dev)
            tmax = t.clone()
            torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.SUM)
            tb, emitted = float(tmax[0].item()), float(t[1].item())
        beam_tok_s = emitted / tb
        beam_ms_per_batch = tb / args.beam_batches * 1e3
        # the reference-compatible regime: the reference cannot tile Bahdanau keys to a beam
        # and runs its RNN beam search one sentence at a time -- the same search at batch 1 here (5 hypothesis rows)
        if rank == 0:
            ones = [synthetic.synthetic_dataset(seed=777 + i, batch=1, src_len=args.length, tgt_len=args.length,
                                                vocab=args.vocab, with_target=False) for i in range(4)]
            for i in range(6):
                tfm.execute(ones[i % 4], runner.feedables, [runner], compute_losses=False)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            n1 = 16
            for i in range(n1):
                tfm.execute(ones[i % 4], runner.feedables, [runner], compute_losses=False)
            torch.cuda.synchronize()
            beam_b1_ms = (time.perf_counter() - t1) / n1 * 1e3
        logit_b[2] = saved_end_bias

    # ---- the other scaling mode in the same run (N > 1): BASELINE.json's wording is the STRONG split (one
    # minibatch of --batch sentences sharded over the GPUs); `value` above is the weak one unless --scaling strong
    other = None
    if dp and world > 1 and args.scaling == "weak" and args.batch % world == 0:
        dp.timing = True
        sb = args.batch // world
        spool = [synthetic.synthetic_dataset(seed=4321 + 1000 * i + rank, batch=sb, src_len=args.length,
                                             tgt_len=args.length, vocab=args.vocab, ragged=False)
                 for i in range(NUM_BATCHES)]
        for b in spool:
            uploader.upload(b)
        for i in range(3):
            step(spool[i % NUM_BATCHES])
        t_strong, _ = timed(spool[i % NUM_BATCHES] for i in range(args.steps))
        t = torch.tensor([t_strong], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        t_strong = float(t.item())
        rep = dp.exchange_report()
        dp.timing = False
        other = {"scaling": "strong", "sentences_per_gpu": sb, "global_batch": args.batch,
                 "ms_per_step": t_strong / args.steps * 1e3,
                 "value": sb * args.length * world * args.steps / t_strong, "unit": "tokens/s",
                 "allreduce_exposed_ms": rep["allreduce_exposed_ms"], "optimizer": rep.get("optimizer"),
                 "optimizer_ms": rep.get("optimizer_ms")}

    # ---- the same step fed from the host inside the timed loop (rank 0 reports; not `value`)
    fresh_ms = strings_ms = None
    if not args.no_feed_legs:
        n = max(8, min(args.steps, 16))
        t_fresh, _ = timed(fresh(pool[i % NUM_BATCHES]) for i in range(n))
        fresh_ms = t_fresh / n * 1e3
        words = model.src_vocab.index_to_word
        spool = [Dataset(d.name, {k: [[words[int(t)] for t in sent] for sent in d.get_series(k)] for k in d.series},
                         d.batching) for d in pool]
        step(fresh(spool[0]))
        t_str, _ = timed(fresh(spool[i % NUM_BATCHES]) for i in range(n))
        strings_ms = t_str / n * 1e3

    # ---- greedy decode + the roofline kernel.  The fused attention step of autoregressive decoding
    # (one query per sentence, B=128, S=50, A=C=1024 -- the "attention-decoder step" of the north
    # star).  Training batches all T steps into one launch, so the step kernel is timed where it
    # really runs once per step: a greedy decode of one 128-sentence batch, 50 steps, launched eagerly
    # with HIP events around the launches of every nm_attn_fwd call on their stream.
    saved_end_bias = float(logit_b[2].item())
    logit_b[2] = -1e9                       # </s> unreachable: all 50 steps run
    dsg = [synthetic.synthetic_dataset(seed=77 + 10 * i + rank, batch=args.batch, src_len=args.length,
                                       tgt_len=args.length, vocab=args.vocab, with_target=False) for i in range(4)]
    grunner = model.greedy_runner
    for i in range(5):                      # warm-up: eager pass + HIP-graph capture pass in both buffer slots
        tfm.execute(dsg[i % 4], grunner.feedables, [grunner], compute_losses=False, lookahead=dsg[(i + 1) % 4])
    barrier()
    tg = time.perf_counter()
    GREEDY_BATCHES = 8
    for i in range(GREEDY_BATCHES):
        nxt = dsg[(i + 1) % 4] if i + 1 < GREEDY_BATCHES else None
        tfm.execute(dsg[i % 4], grunner.feedables, [grunner], compute_losses=False, lookahead=nxt)
    barrier()
    greedy_ms = (time.perf_counter() - tg) * 1e3 / GREEDY_BATCHES
    # the same decode once more with graph replay off, HIP events around every attention step
    sess0 = tfm.sessions[0]
    graphs_were = sess0.use_graphs
    sess0.use_graphs = False
    lib.nm_prof_enable(None, 1)
    tfm.execute(dsg[0], grunner.feedables, [grunner], compute_losses=False)
    barrier()
    lib.nm_prof_enable(None, 0)
    sess0.use_graphs = graphs_were
    logit_b[2] = saved_end_bias
    tot_ms, cnt = ctypes.c_double(0.0), ctypes.c_int64(0)
    lib.nm_prof_attn_step(None, ctypes.byref(tot_ms), ctypes.byref(cnt))
    warm_us, warm_n = (tot_ms.value * 1e3 / cnt.value) if cnt.value else None, cnt.value

    # cold: the same launch at the same shape with a 1 GB sweep in between (evicts the 256 MB Infinity
    # Cache), as inside a training step where 800 MB of logits pass between two uses of the keys
    cold_us = cold_n = dirty_us = None
    if rank == 0:
        a = c = 2 * h
        gen = torch.Generator(device=dev).manual_seed(0)
        y = torch.randn(args.batch, a, device=dev, generator=gen)
        hf = torch.randn(args.batch, args.length, a, device=dev, generator=gen)
        st = torch.randn(args.batch, args.length, c, device=dev, generator=gen)
        mask = torch.ones(args.batch, args.length, device=dev)
        vv = torch.randn(a, device=dev, generator=gen) * 0.05
        bias = torch.zeros(1, device=dev)
        ctx = torch.empty(args.batch, c, device=dev)
        wts = torch.empty(args.batch, args.length, device=dev)
        ws = ops.attn_workspace(args.batch, args.length, c, dev)
        nbytes_of = attention_step_bytes(args.batch, args.length, a, c) // 16 * 16
        flush = torch.zeros(256 << 20, device=dev)                      # 1 GiB of fp32
        sink = torch.zeros(1, device=dev)

        def cold_pass(n, dirty):
            """n launches, each preceded by a sweep over 1 GiB: read-only (the caches are left holding CLEAN
            lines of the sweep) or written (DIRTY lines: the launch then also pays for their write-back)."""
            for i in range(n):
                if dirty:
                    flush.fill_(float(i))
                else:
                    sink.add_(flush.sum())
                ops.attn_fwd(y, hf, st, mask, vv, bias, 1, ctx, wts, ws)
            torch.cuda.synchronize()

        def measure(dirty):
            cold_pass(3, dirty)
            lib.nm_prof_enable(None, 1)
            cold_pass(20, dirty)
            lib.nm_prof_enable(None, 0)
            lib.nm_prof_attn_step(None, ctypes.byref(tot_ms), ctypes.byref(cnt))
            return ((tot_ms.value * 1e3 / cnt.value) if cnt.value else None), cnt.value
        cold_us, cold_n = measure(False)
        dirty_us, _ = measure(True)
        # cold without a sweep in between: NSETS distinct key / value sets (428 MB > the 256 MB Infinity Cache)
        # visited round-robin, launches back to back, ONE event pair around the whole sequence -- every launch reads
        # lines that 7 x 53 MB of other sets have pushed out since its last visit, and the event pair's own cost
        # (event_pair_overhead_us below) is spread over all of them instead of added to each
        NSETS, ROUNDS = 8, 4
        sets = [(hf, st)] + [(torch.randn_like(hf), torch.randn_like(st)) for _ in range(NSETS - 1)]

        def rotate_pass(rounds):
            for i in range(rounds * NSETS):
                khf, kst = sets[i % NSETS]
                ops.attn_fwd(y, khf, kst, mask, vv, bias, 1, ctx, wts, ws)
        rotate_pass(1)
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        rotate_pass(ROUNDS)
        ev1.record()
        torch.cuda.synchronize()
        rot_us = ev0.elapsed_time(ev1) * 1e3 / (ROUNDS * NSETS)
        rot_n = ROUNDS * NSETS
        # the same sequence for the streaming yardstick
        probes = [torch.randn(nbytes_of // 4, device=dev, generator=gen) for _ in range(NSETS)]
        psink0 = torch.zeros(2048, device=dev)

        def rotate_stream(rounds):
            for i in range(rounds * NSETS):
                _lib.check(lib.nm_prof_stream_read(ops._stream(), probes[i % NSETS].data_ptr(), nbytes_of,
                                                   psink0.data_ptr()), "nm_prof_stream_read")
        rotate_stream(1)
        torch.cuda.synchronize()
        ev0.record()
        rotate_stream(ROUNDS)
        ev1.record()
        torch.cuda.synchronize()
        rot_stream_us = ev0.elapsed_time(ev1) * 1e3 / (ROUNDS * NSETS)
        del sets, probes
        # yardstick: the same number of bytes read cold by a plain streaming kernel (nm_prof_stream_read), same
        # sweep in between, same event pool -- what ONE launch of this size can reach on this part
        nbytes = attention_step_bytes(args.batch, args.length, a, c) // 16 * 16
        probe = torch.randn(nbytes // 4, device=dev, generator=gen)
        psink = torch.zeros(2048, device=dev)

        def stream_pass(n):
            for _ in range(n):
                sink.add_(flush.sum())
                _lib.check(lib.nm_prof_stream_read(ops._stream(), probe.data_ptr(), nbytes, psink.data_ptr()),
                           "nm_prof_stream_read")
            torch.cuda.synchronize()
        stream_pass(3)
        lib.nm_prof_enable(None, 1)
        stream_pass(20)
        lib.nm_prof_enable(None, 0)
        lib.nm_prof_attn_step(None, ctypes.byref(tot_ms), ctypes.byref(cnt))
        stream_us = (tot_ms.value * 1e3 / cnt.value) if cnt.value else None
        # what the event pair itself costs: the same protocol around a 4-thread-block's worth of work (16 bytes)
        def empty_pass(n):
            for _ in range(n):
                sink.add_(flush.sum())
                _lib.check(lib.nm_prof_stream_read(ops._stream(), probe.data_ptr(), 16, psink.data_ptr()),
                           "nm_prof_stream_read")
            torch.cuda.synchronize()
        empty_pass(3)
        lib.nm_prof_enable(None, 1)
        empty_pass(20)
        lib.nm_prof_enable(None, 0)
        lib.nm_prof_attn_step(None, ctypes.byref(tot_ms), ctypes.byref(cnt))
        overhead_us = (tot_ms.value * 1e3 / cnt.value) if cnt.value else None
        del flush, probe

    if rank == 0:
        a = c = 2 * h
        step_bytes = attention_step_bytes(args.batch, args.length, a, c)
        gbps = lambda us: (step_bytes / (us * 1e-6) / 1e9) if us else None
        warm, cold, rot = gbps(warm_us), gbps(cold_us), gbps(rot_us)
        traffic = pmc_kernels = None
        pmc = newest_profile("r[0-9][0-9]_attn_step_pmc_cold.json") or os.path.join(ROOT, "profiles", "attn_step_pmc.json")
        if os.path.exists(pmc):
            with open(pmc) as fh:
                rec = json.load(fh)
            traffic, pmc_kernels = rec.get("hbm_bytes_per_launch"), rec.get("kernels")
        # rocprofv3 kernel durations of the same launches (committed summaries of separate profiled runs:
        # tools/attn_evidence.sh, the newest round's files)
        rocprof_us, rocprof_files = {}, []
        for mode in ("cold", "warm", "dirty"):
            path = newest_profile("r[0-9][0-9]_attn_step_trace_{}.json".format(mode)) or \
                os.path.join(ROOT, "profiles", "r02_attn_step_trace_{}_v4.json".format(mode))
            if os.path.exists(path):
                with open(path) as fh:
                    rocprof_us[mode] = json.load(fh).get("sum_avg_us")
                rocprof_files.append(os.path.relpath(path, ROOT))
        dstep_bytes = decoder_step_bytes(args.batch, args.length, h, args.vocab)
        dstep_us = greedy_ms * 1e3 / args.length
        fields = {
            "other_scaling": other,
            "ms_per_step_fresh": fresh_ms, "ms_per_step_strings": strings_ms,
            "beam5_decode_tok_s": beam_tok_s, "beam5_ms_per_batch": beam_ms_per_batch,
            "beam5_batch1_ms_per_sentence": beam_b1_ms,
            "beam5_batch1_tok_s": (args.length / (beam_b1_ms * 1e-3)) if beam_b1_ms else None,
            "greedy_decode_tok_s": tokens_local / (greedy_ms * 1e-3), "greedy_ms_per_batch": greedy_ms,
            "roofline": {"kernel": "nm_attn_fwd = attn_whole_fast<13>, ONE launch (fused Bahdanau score + softmax + "
                                   "mask-renorm + context of one decoding step; one 1024-thread workgroup per sentence: "
                                   "no split-S partials, no merge; smaller batches / longer sources take the split-S "
                                   "kernel with its in-kernel merge)",
                         "timing": "HIP events on the launch stream (the library's recorder around single calls, one "
                                   "torch.cuda.Event pair -- torch's current stream IS the launch stream -- around the "
                                   "back-to-back sequence); rocprofv3 kernel durations of the same kernel: {}, "
                                   "repeated in rocprof_kernel_us".format(", ".join(rocprof_files)),
                         "bound": "hbm", "achieved": rot, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": (rot / HBM_PEAK_GBPS) if rot else None, "traffic": traffic,
                         "traffic_how": "HBM bytes per launch from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE "
                                        "passes (gfx950 wide-read correction applied), read from the committed "
                                        "{} -- NOT counted during this run".format(os.path.relpath(pmc, ROOT)),
                         "achieved_how": "cold, back to back: {} launches over {} distinct key / value sets (428 MB, "
                                         "round-robin: a set's lines are evicted from L2 and the 256 MB Infinity Cache "
                                         "before its next visit), ONE HIP-event pair on the launch stream around the "
                                         "sequence; {:.2f} us per launch".format(rot_n, NSETS, rot_us),
                         "cold_rotating_launch_us": rot_us,
                         "stream_read_rotating_us": rot_stream_us,
                         "frac_of_stream_read_rotating": (rot_stream_us / rot_us) if rot_us else None,
                         "traffic_kernels": pmc_kernels,
                         "rocprof_kernel_us": rocprof_us or None,
                         "frac_rocprof_cold": (step_bytes / (rocprof_us["cold"] * 1e-6) / 1e9 / HBM_PEAK_GBPS)
                         if rocprof_us.get("cold") else None,
                         "achieved_cold": cold, "frac_cold_single": (cold / HBM_PEAK_GBPS) if cold else None,
                         "cold_launch_us": cold_us, "cold_launches": cold_n,
                         "cold_how": "ONE launch between two events, a 1 GiB read sweep before it (L2 + 256 MB Infinity "
                                     "Cache evicted, clean lines): includes what the event pair itself costs "
                                     "(event_pair_overhead_us)",
                         "cold_dirty_launch_us": dirty_us,
                         "cold_dirty_how": "the same with a 1 GiB WRITE sweep: the caches hold dirty lines whose "
                                           "write-back competes with the kernel's reads",
                         "stream_read_cold_us": stream_us,
                         "stream_read_how": "yardstick: the same {} bytes read cold by a plain float4 streaming kernel "
                                            "(nm_prof_stream_read), same sweep, same events; cold_launch_us / this = "
                                            "how far the step kernel is from what one launch of this size can "
                                            "reach".format(step_bytes // 16 * 16),
                         "frac_of_stream_read": (stream_us / cold_us) if (stream_us and cold_us) else None,
                         "event_pair_overhead_us": overhead_us,
                         "event_pair_overhead_how": "the same event pair around a launch that reads 16 bytes: what of "
                                                    "cold_launch_us is dispatch + event latency rather than kernel",
                         "achieved_warm": warm, "frac_warm": (warm / HBM_PEAK_GBPS) if warm else None,
                         "warm_launch_us": warm_us, "warm_launches": warm_n,
                         "warm_how": "inside a greedy decode of one B={} batch, {} steps, launched eagerly".format(
                             args.batch, args.length),
                         "algorithmic_bytes_per_launch": step_bytes},
            "roofline_step": {"what": "one greedy decoder step (GRU + attention + output projection + logits + "
                                      "argmax), HIP-graph replayed", "bound": "hbm",
                              "algorithmic_bytes_per_step": dstep_bytes, "us_per_step": dstep_us,
                              "achieved": dstep_bytes / (dstep_us * 1e-6) / 1e9, "peak": HBM_PEAK_GBPS,
                              "unit": "GB/s", "frac": dstep_bytes / (dstep_us * 1e-6) / 1e9 / HBM_PEAK_GBPS},
        }
        if world == 1 and not args.no_configs:
            # free the headline model's buffers first: the legs build their own sessions
            legs = {}
            for name, fn in (("transformer", lambda: transformer_leg(args, dev)),
                             ("captioning", lambda: captioning_leg(args, dev, lib)),
                             ("general_path", lambda: general_path_leg(args, dev)),
                             ("gru_time_loops", lambda: time_loops_leg(args, dev)),
                             ("decode_split_projection", lambda: split_projection_leg(args, dev)),
                             ("logits_gemm_bf16x3", lambda: bf16x3_costing_leg(args, dev, lib))):
                try:
                    legs[name] = fn()
                except Exception as exc:                  # pragma: no cover  (never hide the headline number)
                    legs[name] = {"error": repr(exc)}
            fields["configs"] = legs
        if world == 1 and not args.no_cpu_baseline:
            try:
                fields["cpu_baseline"] = cpu_baseline(args)
            except Exception as exc:                      # pragma: no cover  (never hide the GPU number)
                fields["cpu_baseline"] = {"value": None, "error": repr(exc)}
        return fields
    return None


def main():
    args = parse()
    from neuralmonkey_amd import _lib, distributed, synthetic
    from neuralmonkey_amd.dataset import Dataset
    from neuralmonkey_amd.input_pipeline import Prefetcher
    dp = distributed.init_from_env()
    rank = dp.rank if dp else 0
    world = dp.world_size if dp else 1
    if world != args.gpus:
        raise SystemExit("--gpus {} but WORLD_SIZE={}".format(args.gpus, world))
    # one rank per GPU; ranks beyond the visible devices wrap around (only meaningful with
    # NM_DIST_BACKEND=gloo, the single-GPU smoke test of the multi-rank code path)
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = "cuda:{}".format(local)
    lib = _lib.load()
    if args.scaling == "strong":
        if args.batch % world:
            raise SystemExit("--scaling strong: --batch {} is not divisible by {} GPUs".format(args.batch, world))
        args.batch //= world                  # from here on: sentences per GPU

    h = args.hidden
    model = synthetic.build_translation_model(vocab_src=args.vocab, vocab_tgt=args.vocab, emb=h, rnn=h,
                                              max_len=args.length, beam_size=5, max_steps=args.length,
                                              length_normalization=0.6, l2_weight=1e-8, clip_norm=1.0,
                                              device=dev, seed=1234)
    store = model.tf_manager.sessions[0].store
    synthetic.load_baseline_weights(store, seed=1234, std=0.05)
    if dp:
        dp.broadcast_parameters(store)
    tfm, trainer = model.tf_manager, model.trainer
    feedables = trainer.feedables
    # NUM_BATCHES distinct batches of pre-indexed int32 ids per rank
    pool = [synthetic.synthetic_dataset(seed=1234 + 1000 * i + rank, batch=args.batch, src_len=args.length,
                                        tgt_len=args.length, vocab=args.vocab, ragged=False)
            for i in range(NUM_BATCHES)]
    tokens_local = args.batch * args.length               # every target has len-1 tokens + </s>
    tokens_global = tokens_local * world

    def fresh(d):
        """The same data as a NEW batch object: no feed dict cached on it, nothing resident in HBM."""
        return Dataset(d.name, {k: list(d.get_series(k)) for k in d.series}, d.batching)

    def step(batch):
        return tfm.execute(batch, feedables, [trainer], train=True)[0]

    def barrier():
        if dp:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    def timed(batches):
        barrier()
        t0 = time.perf_counter()
        for b in batches:
            out = step(b)
        barrier()
        return time.perf_counter() - t0, out

    # ---- training: the headline number.  All NUM_BATCHES batches are uploaded first (feed dicts built,
    # ids resident in HBM), then W warm-up steps (>= 2: eager pass with allocations + HIP-graph capture
    # pass), then EXACTLY K timed steps rotating through the distinct batches.
    uploader = Prefetcher(tfm, feedables, train=True)
    for b in pool:
        uploader.upload(b)
    for i in range(max(args.warmup, 2)):
        step(pool[i % NUM_BATCHES])
    if dp:
        dp.timing = True
        dp.exchange_report()
    elapsed, res = timed(pool[i % NUM_BATCHES] for i in range(args.steps))
    dp_report = None
    if dp:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
        dp_report = dp.exchange_report()
        dp_report["how"] = ("allreduce_exposed_ms: HIP events on rank 0's compute stream around the point where the "
                            "optimizer has to wait for the gradient collectives (mean over the timed steps) = the part "
                            "of the exchange that the backward pass did not hide; bytes: flat gradient buffer per "
                            "step and rank, early_bytes: the spans whose collective starts inside the backward pass; "
                            "optimizer: 'sharded' = reduce-scatter -> clip + Adam on this rank's slices of the flat "
                            "buffers -> all-gather of the parameters (NM_DP_SHARDED=0: all-reduce + the whole update on "
                            "every rank); optimizer_ms: HIP events around norms + update (+ all-gather); "
                            "exchanged_bytes_per_rank: what a rank sends per step with ring collectives")
        dp.timing = False
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, res)
    extra = full_legs(args, dp, rank, world, dev, lib, model, tfm, pool, uploader, step, timed, fresh,
                      barrier) if args.full else None

    if rank == 0:
        line = {
            "metric": "target tokens/sec/node (train), 512-hid GRU+attn",
            "value": tokens_global * args.steps / elapsed, "unit": "tokens/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": args.scaling,
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "translation.ini-shape: biGRU-{h} enc + Bahdanau attn + GRU-{h} dec, "
                                   "B={b}/GPU, src_len=tgt_len={l}, V={v}, weights N(0,0.05)/orthogonal "
                                   "(BASELINE.md 3), CrossEntropyTrainer(l2=1e-8, clip_norm=1.0) + Adam(1e-4), "
                                   "one optimizer step per step, {n} distinct HBM-resident batches in "
                                   "rotation".format(h=h, b=args.batch, l=args.length, v=args.vocab, n=NUM_BATCHES),
                       "global_batch": args.batch * world, "seq_len": args.length,
                       "parallelism": "dp{}".format(world)},
            "loss": res.losses["decoder - cost"],
            "dp": dp_report,
            "roofline_train": (lambda fl, sec: {
                "what": "the timed region of `value`: one whole training step (forward, backward, clip, Adam) against "
                        "the fp32 matrix-core peak; flops = 2 x multiply-adds of every dense product, forward + "
                        "backward (synthetic.translation_train_flops: the Bahdanau energies / contexts on the vector "
                        "units are not counted)",
                "bound": "mfma", "flops_per_step": fl, "achieved": fl / sec / 1e12, "peak": MFMA_F32_PEAK_TF,
                "unit": "TFLOP/s", "frac": fl / sec / 1e12 / MFMA_F32_PEAK_TF})(
                    synthetic.translation_train_flops(args.batch, args.length, args.vocab, h), elapsed / args.steps),
        }
        line.update(extra or {})
        print(json.dumps(line), flush=True)
    if dp:
        distributed.shutdown()


if __name__ == "__main__":
    main()
