"""Truncated sampling as a decoding mode: temperature, top-k and nucleus (top-p) sampling, several samples per
sentence, a log-probability for each sample.

The reference has no such decoder: its only stochastic decoding is the bare ``tf.multinomial`` loop of
decoders/autoregressive.py:470-473, one draw per sentence over the whole vocabulary, reachable from the RL trainers
only (``AutoregressiveDecoder.decoding_loop(sample=True)`` here, unchanged).  ``SamplingDecoder`` wraps any parent with
a stepwise inference interface (``make_stepper``) the way ``BeamSearchDecoder`` does: the initial state is tiled to
``num_samples`` rows per sentence (row ``b * n + j`` reads the keys of sentence ``b``), and every step is

    nm_sample_step (csrc/nm_sample.hip: kept set, draw, log-probability, loop state)
    -> embed the drawn symbols -> parent decoder step -> new logits.

Rows never change parents, so nothing is reordered.  The draw's salt is ``word + step * const``: the word lives on the
device and is rewritten in front of every run, outside the captured chunks, so a replayed graph draws afresh; the
salts are the parent's ``sampling_salts`` (session seed, decoder name, loop counter), so a seeded session reproduces.
"""
from typing import Any, List, NamedTuple

import torch

from .. import ops
from ..model.model_part import ModelPart
from ..runtime import Placeholder, tensor
from ..vocabulary import END_TOKEN_INDEX, START_TOKEN_INDEX, Vocabulary
from .autoregressive import AutoregressiveDecoder
from .decoder import CHECK_EVERY_BEAM

MAX_NUM_SAMPLES = 64      # the attention entries' rows_per_key <= 64
SALT_STEP = 0x632BE5AB    # AutoregressiveDecoder.sampling_salts: salt of step t = salt of step 0 + t * SALT_STEP


class SamplingOutput(NamedTuple):
    token_ids: torch.Tensor          # [steps, B, n] int32: the drawn symbols, <pad> after </s>
    logprob_sum: torch.Tensor        # [B, n] log-probability of every sample under the distributions drawn from
    lengths: torch.Tensor            # [B, n] int32 (</s> included)
    finished: torch.Tensor           # [B, n] int32 (0/1)


class SamplingDecoder(ModelPart):
    def __init__(self, name: str, parent_decoder: AutoregressiveDecoder, max_steps: int, num_samples: int = 1,
                 temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0) -> None:
        ModelPart.__init__(self, name)
        self.parent_decoder = parent_decoder
        self.num_samples = num_samples
        self.temperature = float(temperature)
        self.top_k = top_k
        self.top_p = float(top_p)
        self.max_steps_int = max_steps
        self.keep_logits = False          # checks: keep every step's logits (``step_records``)
        if num_samples < 1 or num_samples > MAX_NUM_SAMPLES:
            raise ValueError("num_samples must be between 1 and {} (every sample is a row of its sentence's attention "
                             "keys, and the attention kernels take rows_per_key <= {}), was {}"
                             .format(MAX_NUM_SAMPLES, MAX_NUM_SAMPLES, num_samples))
        if not self.temperature > 0.0 or self.temperature == float("inf"):
            raise ValueError("temperature must be positive and finite, got {}".format(temperature))
        if top_k < 0:
            raise ValueError("top_k must be >= 0 (0: no top-k truncation), got {}".format(top_k))
        if not 0.0 < self.top_p <= 1.0:
            raise ValueError("top_p must be in (0, 1] (1: no nucleus truncation), got {}".format(top_p))
        if max_steps < 1:
            raise ValueError("max_steps must be at least 1, got {}".format(max_steps))
        if not hasattr(parent_decoder, "make_stepper"):
            raise NotImplementedError("SamplingDecoder: parent decoder '{}' has no stepwise inference "
                                      "interface (make_stepper)".format(type(parent_decoder).__name__))
        self.max_steps = Placeholder("{}/max_steps".format(name), default=max_steps)

    @property
    def vocabulary(self) -> Vocabulary:
        return self.parent_decoder.vocabulary

    def expand_index(self, ctx, bsz: int) -> torch.Tensor:
        """Row r of the tiled batch continues sentence r // n."""
        key = (id(self), "expand", bsz)
        if key not in ctx.session.__dict__.setdefault("_const", {}):
            idx = torch.arange(bsz * self.num_samples, dtype=torch.int32) // self.num_samples
            ctx.session._const[key] = idx.to(torch.int32).to(ctx.device)
        return ctx.session._const[key]

    @tensor
    def outputs(self, ctx) -> SamplingOutput:
        dec = self.parent_decoder
        for att in dec.attentions:
            att.rows_per_key = self.num_samples
        try:
            return self._sample(ctx)
        finally:
            for att in dec.attentions:
                att.rows_per_key = 1

    def ensemble_outputs(self, ctxs: List[Any]) -> SamplingOutput:
        if len(ctxs) > 1:
            raise NotImplementedError("SamplingDecoder: sampling from an ensemble ({} sessions) is not implemented"
                                      .format(len(ctxs)))
        return self.outputs(ctxs[0])

    @tensor
    def step_records(self, ctx):
        """(logprob [steps, B, n], kept [steps, B, n], logits [steps, B * n, V] or None) of the executed steps: what a
        check needs beside ``outputs``."""
        self.outputs(ctx)
        return ctx.memo[(id(self), "_step_records")]

    def _sample(self, ctx) -> SamplingOutput:
        from ..attention.base_attention import AttentionLoopState
        dec, n = self.parent_decoder, self.num_samples
        bsz = int(ctx.fed(dec.batch_size))
        rows = bsz * n
        e, v = dec.embedding_size or dec.output_dimension, len(self.vocabulary)
        max_steps = int(ctx.fed(self.max_steps))
        keep = bool(self.keep_logits)
        key = (id(self), "smp", bsz, keep)
        f32 = lambda name, shape, **kw: ctx.buffer(key + (name,), shape, torch.float32, **kw)
        i32 = lambda name, shape, **kw: ctx.buffer(key + (name,), shape, torch.int32, **kw)

        stepper = dec.make_stepper(ctx, rows, "sample", n, max_positions=max_steps + 1)
        emb = getattr(stepper, "emb_view", None)          # embed straight into the stepper's input slot
        if emb is None:
            emb = f32("emb", (rows, e))
        out_state = f32("out", (rows, dec.output_dimension))
        logits_all = f32("logits", (max_steps + 1 if keep else 1, rows, v))
        logits_at = (lambda i: logits_all[i]) if keep else (lambda i: logits_all[0])
        tok = i32("tok", (max_steps, rows))               # the drawn symbols ARE the token history
        lp_hist = f32("lp_hist", (max_steps, rows))
        kept_hist = i32("kept_hist", (max_steps, rows))
        lps, lens, fin = f32("lps", (2, rows)), i32("lens", (2, rows)), i32("fin", (2, rows))
        allfin = i32("allfin", (max_steps,))
        ops.fill(allfin, 1)
        salt_word = i32("salt", (1,))
        att0 = [a.initial_loop_state(ctx, rows, max_steps + 1) for a in dec.attentions]
        att_at = lambda i: [AttentionLoopState(a.contexts, a.weights, i) for a in att0]

        # the salts of this run: step t draws with salts[t] = salts[0] + t * SALT_STEP; the first one goes into the
        # device word (a launch outside the captured chunks), the multiples of SALT_STEP are baked into the launches
        salts = dec.sampling_salts(ctx, max_steps)
        assert all((salts[0] + t * SALT_STEP) & 0xFFFFFFFF == s for t, s in enumerate(salts))
        ctx.memo[(id(self), "sampling_salts")] = salts
        ops.fill(salt_word, salts[0] - (1 << 32) if salts[0] >= (1 << 31) else salts[0])

        fast = getattr(stepper, "graph_safe", False)      # steps keep no Python-side state: HIP-graph capturable
        indexed = getattr(stepper, "indexed", False)      # steps are a function of an explicit position: also capturable
        resident = getattr(stepper, "state_resident", False)
        tabled = fast and getattr(stepper, "table", None) is not None       # input tables: steps take symbols
        go = i32("go", (rows,))
        hsel = s0 = None
        if hasattr(dec, "initial_state"):                 # RNN decoder: tile the initial state
            hsel = f32("hsel", (rows, dec.rnn_size))
            s0 = dec.initial_state(ctx)
        expand = self.expand_index(ctx, bsz)
        loop = {"att": att0}

        def initial_step():
            """Tile, feed <s>, run the parent step once: persistent buffers only."""
            if hsel is not None:
                ops.gather_rows(s0, expand, hsel)
                stepper.start(hsel)
            else:
                stepper.start()
            ops.zero(fin[0])
            ops.zero(lps[0])
            ops.zero(lens[0])
            ops.fill(go, START_TOKEN_INDEX)
            if not tabled:
                dec.embed_input_symbols(ctx, go, out=emb)
            if fast:
                stepper.step(emb, att_at(0), out_state, logits_at(0), h_prev=hsel, h_out=stepper.hbuf[0],
                             **({"ids": go} if tabled else {}))
            else:
                loop["att"] = stepper.step(emb, att0, out_state, logits_at(0), finished=fin[0])
        if fast:
            for att in dec.attentions:                    # lazily built tensors (H2D copies): outside the capture
                att.hidden_features(ctx)
                att.attention_mask(ctx)
            dec.decoding_bias(ctx)
            ctx.session.graphed(key + ("init", n, v, tuple(tuple(a.weights.shape) for a in att0),
                                       getattr(stepper, "shape_key", ()), 0 if s0 is None else s0.data_ptr(),
                                       bool(tabled)), initial_step)
        else:
            initial_step()

        def body(s):
            """Step s: draw from the logits of position s, advance the parent to position s + 1; every buffer it
            touches is a function of s alone."""
            cur, nxt = s & 1, (s & 1) ^ 1
            ops.sample_step(logits_at(s), salt_word, s * SALT_STEP, END_TOKEN_INDEX, fin[cur], lps[cur], lens[cur],
                            tok[s], lp_hist[s], kept_hist[s], fin[nxt], lps[nxt], lens[nxt],
                            temperature=self.temperature, top_k=self.top_k, top_p=self.top_p,
                            all_finished=allfin[s:s + 1])
            if not tabled:
                dec.embed_input_symbols(ctx, tok[s], out=emb)
            if fast:
                stepper.step(emb, att_at(s + 1), out_state, logits_at(s + 1),
                             h_prev=stepper.sel if resident else stepper.hbuf[cur], h_out=stepper.hbuf[nxt],
                             **({"ids": tok[s]} if tabled else {}))
            elif indexed:
                stepper.set_position(s + 1, 0)
                stepper.step(emb, att_at(s + 1), out_state, logits_at(s + 1), finished=fin[nxt])
            else:
                loop["att"] = stepper.step(emb, loop["att"], out_state, logits_at(s + 1), finished=fin[nxt])

        graphed = fast or indexed
        chunk_key = key + ("chunk", n, v, tuple(tuple(a.weights.shape) for a in att0),
                           getattr(stepper, "shape_key", ()), self.temperature, self.top_k, self.top_p)

        def launch(first, count):
            def chunk():
                for s in range(first, first + count):
                    body(s)
            if graphed:
                ctx.session.graphed(chunk_key + (first, count), chunk)
            else:
                chunk()
        steps, executed = ctx.session.decode_chunks(max_steps, CHECK_EVERY_BEAM, launch, allfin, run_ahead=graphed)
        cur = executed & 1                                # buffers the last executed body wrote
        ctx.memo[(id(self), "_step_records")] = (lp_hist[:steps].view(steps, bsz, n),
                                                 kept_hist[:steps].view(steps, bsz, n),
                                                 logits_all[:steps] if keep else None)
        return SamplingOutput(tok[:steps].view(steps, bsz, n), lps[cur].view(bsz, n), lens[cur].view(bsz, n),
                              fin[cur].view(bsz, n))
