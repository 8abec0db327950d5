"""SamplingDecoder (temperature, top-k and nucleus sampling, several samples per sentence) over its three kinds of
parent: the RNN decoder on the fast path, a conditional-GRU decoder on the general path, a 2-layer Transformer.
B = 6 sentences, n = 3 samples, V = 300, width 32, at most 10 steps.

The engine's draws are handed back to the CPU oracle (teacher forcing, as tests/test_sampling_gpu.py does): the oracle's
logits must be the engine's (1e-4 of their largest magnitude), and every draw of a live row must belong to the kept
set computed from the ORACLE's logits with the boundary moved outward by that tolerance.  Finished rows emit <pad>,
``logprob_sum`` is the float32 sum of the per-step values in step order, the samples of a sentence differ, a second
run draws differently, a session rebuilt with the same seed draws the same, ``top_k = 1`` is the greedy decoder, the
runner's sentences and loss are those of ``outputs``, and a step launches no ``at::native`` kernel."""
import numpy as np
import pytest
import torch

from oracle import general_ref as G
from oracle import nm_oracle as O
from oracle import transformer_ref as TRF

from . import sampling_ref as SR

pytestmark = pytest.mark.gpu

VOCAB, WIDTH, BATCH, N, STEPS = 300, 32, 6, 3, 10
TEMPERATURE, TOP_K, TOP_P = 0.9, 40, 0.9
LOGIT_TOL = 1e-4


def _sampler(parent, name="sampler", **kw):
    from neuralmonkey_amd.decoders import SamplingDecoder
    args = dict(num_samples=N, temperature=TEMPERATURE, top_k=TOP_K, top_p=TOP_P)
    args.update(kw)
    return SamplingDecoder(name=name, parent_decoder=parent, max_steps=STEPS, **args)


# ---- the three parents: (session, feed dict, parent decoder, teacher-forced oracle logits) ------------------------------
def _rnn_fast(dev, seed=7):
    from tests.test_engine_gpu import _setup
    model, params, ds, src, _ = _setup(dev, VOCAB, WIDTH, WIDTH, BATCH, 9, STEPS, True, beam=0, std=0.3, seed=seed)
    fd = {}
    for f in model.greedy_runner.feedables:
        fd.update(f.feed_dict(ds, train=False))

    def forced_logits(sym, n):
        enc = O.sentence_encoder(params, np.repeat(src, n, axis=0))
        spec = O.DecoderSpec(max_output_len=STEPS)
        forced = np.zeros((STEPS, sym.shape[1]), np.int64)
        forced[:len(sym)] = sym
        return O.decoding_loop(params, spec, enc, forced, True).logits[:len(sym)]
    return dict(model=model, tfm=model.tf_manager, fd=fd, dec=model.decoder, forced_logits=forced_logits, ds=ds,
                params=params, src=src)


GENERAL_CFG = G.Config(rnn_layers=((16, "bidirectional", "GRU"),), dec_cell="GRU", conditional_gru=True, rnn_size=WIDTH,
                       output_projection=("nonlinear", "tanh", 1.0))


def _general(dev, seed=5):
    from neuralmonkey_amd import synthetic
    from neuralmonkey_amd.attention import Attention
    from neuralmonkey_amd.decoders import Decoder
    from neuralmonkey_amd.decoders import output_projection as OP
    from neuralmonkey_amd.encoders import RecurrentEncoder
    from neuralmonkey_amd.model.sequence import EmbeddedSequence
    from neuralmonkey_amd.runtime import reset_registry
    from neuralmonkey_amd.tf_manager import TensorFlowManager
    cfg = GENERAL_CFG
    reset_registry()
    vocab = synthetic.synthetic_vocabulary(VOCAB)
    seq = EmbeddedSequence(name=cfg.enc_name + "_input", vocabulary=vocab, data_id="source", embedding_size=WIDTH,
                           max_length=STEPS)
    enc = RecurrentEncoder(name=cfg.enc_name, input_sequence=seq, rnn_layers=[tuple(l) for l in cfg.rnn_layers])
    att = Attention(name=cfg.att_name, encoder=enc)
    act = type("Act", (), {"nm_name": "tanh"})()
    dec = Decoder(encoders=[enc], vocabulary=vocab, data_id="target", name=cfg.dec_name, max_output_len=STEPS,
                  embedding_size=WIDTH, rnn_size=WIDTH, output_projection=OP.nonlinear_output(WIDTH, act, 1.0),
                  attentions=[att], rnn_cell="GRU", conditional_gru=True, dropout_keep_prob=cfg.dec_dropout,
                  attention_on_input=cfg.attention_on_input, supress_unk=cfg.supress_unk,
                  tie_embeddings=cfg.tie_embeddings)
    tfm = TensorFlowManager(num_sessions=1, num_threads=1, device=str(dev), seed=seed)
    tfm.initialize_sessions()
    store = tfm.sessions[0].store
    rng = np.random.default_rng(seed)
    vals = store.state_dict()
    for name, v in vals.items():
        if v.ndim >= 2 or name.endswith("attn_similarity_v"):
            vals[name] = (rng.standard_normal(v.shape) * 0.3).astype(np.float32)
    store.load_state_dict(vals)
    params = store.state_dict()
    ds = synthetic.synthetic_dataset(seed=3, batch=BATCH, src_len=8, tgt_len=7, vocab=VOCAB, ragged=True,
                                     with_target=False)
    src = O.pad_ids([list(s) for s in ds.get_series("source")], STEPS)
    fd = {}
    for part in (seq, enc, att, dec):
        fd.update(part.feed_dict(ds, train=False))
    assert dec.uses_general_path(False)

    def forced_logits(sym, n):
        ref = G.GeneralModel(params, cfg)
        with torch.no_grad():
            st, hf, mask, state = ref._decode_setup(src, n)              # pylint: disable=protected-access
            table = ref.p[cfg.dec_name + "/word_embeddings"]
            emb = table[torch.full((sym.shape[1],), O.START)]
            hist = []
            for t in range(len(sym)):
                out, state, _ = ref.decoder_step(emb, state, st, hf, mask, False, t)
                hist.append(ref.logits(out).numpy())
                emb = table[torch.as_tensor(sym[t].astype(np.int64))]
        return np.stack(hist)
    return dict(tfm=tfm, fd=fd, dec=dec, forced_logits=forced_logits, ds=ds)


def _transformer(dev, seed=5):
    from tests.test_transformer_gpu import _build, _data
    cfg = TRF.TConfig(depth=2, n_heads=2, n_heads_self=2, n_heads_enc=2)
    m = _build(dev, cfg, WIDTH, 48, max_len=STEPS, beam=2, seed=seed, init_std=0.6, vocab_size=VOCAB)
    ds, src, _ = _data(BATCH, 7, 6, STEPS, seed=8, with_target=False, vocab_size=VOCAB)
    fd = {}
    for part in (m["enc"].input_sequence, m["enc"], m["dec"]):
        fd.update(part.feed_dict(ds, train=False))

    def forced_logits(sym, n):
        model = TRF.TransformerModel(m["params"], cfg)
        _, _, logits = model.greedy(np.repeat(src, n, axis=0), STEPS,
                                    pick=lambda t, lg: sym[t] if t < len(sym) else lg.argmax(1))
        return logits[:len(sym)]
    return dict(tfm=m["tfm"], fd=fd, dec=m["dec"], forced_logits=forced_logits, ds=ds)


PARENTS = {"rnn_fast": _rnn_fast, "general_cond_gru": _general, "transformer": _transformer}


def _run(sess, fd, sdec):
    from neuralmonkey_amd.runtime import RunContext
    ctx = RunContext(sess, fd)
    with torch.no_grad():
        out = sdec.outputs(ctx)
        lp, kept, logits = sdec.step_records(ctx)
        host = lambda t: None if t is None else t.detach().cpu().numpy().copy()
        res = dict(tok=host(out.token_ids), lps=host(out.logprob_sum), lens=host(out.lengths), fin=host(out.finished),
                   lp=host(lp), kept=host(kept), logits=host(logits), salts=list(ctx.memo[(id(sdec), "sampling_salts")]))
    return res


def _check_against_oracle(res, ref_logits, temperature, top_k, top_p):
    """Rows are b * n + j.  Returns the share of draws that are exactly the restated draw over the oracle's kept set."""
    steps, bsz, n = res["tok"].shape
    rows = bsz * n
    sym = res["tok"].reshape(steps, rows)
    lp, kept = res["lp"].reshape(steps, rows), res["kept"].reshape(steps, rows)
    scale = float(np.abs(ref_logits).max())
    assert float(np.abs(res["logits"] - ref_logits).max()) < LOGIT_TOL * scale
    inv_t = np.float32(1.0 / temperature)
    eps = LOGIT_TOL * scale * float(inv_t)               # what a z of the engine may differ from the oracle's by
    finished = np.zeros(rows, bool)
    lps = np.zeros(rows, np.float32)
    lens = np.zeros(rows, np.int32)
    exact = total = 0
    for t in range(steps):
        ref = SR.ref_step(ref_logits[t], inv_t, top_k, top_p, res["salts"][t], O.END, finished, lps, lens)
        for r in range(rows):
            if finished[r]:
                assert (sym[t, r], lp[t, r], kept[t, r]) == (0, 0.0, 0), (t, r)       # <pad> once a row has emitted </s>
                continue
            z = ref.z[r].astype(np.float64)
            ahead = z > z[sym[t, r]] + 2 * eps           # certainly in front of the draw in the engine's order too
            assert ahead.sum() < ref.kk, (t, r)
            if top_p < 1.0:
                mass = np.exp(z[ahead] - ref.zmax[r]).sum()
                assert mass < ref.top_p * ref.mass[r] * (1 + 4 * eps + 1e-5), (t, r)
            k = int(kept[t, r])
            assert 1 <= k <= ref.kk, (t, r, k)
            want_lp = (z[sym[t, r]] - ref.zmax[r]) - np.log(ref.cum[r, k - 1])
            assert abs(lp[t, r] - want_lp) <= 2 * eps + 1e-5, (t, r)      # over the engine's own prefix size
            prefix = ref.order[r, :int(ref.kept[r])]
            noisy = (ref.z[r][prefix] + ref.noise[r][prefix]).astype(np.float32)
            exact += int(prefix[noisy.argmax()] == sym[t, r])
            total += 1
        lps = lps + lp[t]                                # float32, step order: what the kernel adds
        lens = lens + (~finished).astype(np.int32)
        finished = finished | (sym[t] == O.END)
    assert np.array_equal(res["lps"].reshape(rows), lps)
    assert np.array_equal(res["lens"].reshape(rows), lens)
    assert np.array_equal(res["fin"].reshape(rows), finished.astype(np.int32))
    return exact / max(total, 1)


@pytest.mark.parametrize("parent", sorted(PARENTS))
def test_sampling_loop_against_the_oracle(dev, parent):
    p = PARENTS[parent](dev)
    sdec = _sampler(p["dec"])
    sdec.keep_logits = True
    sess = p["tfm"].sessions[0]
    res = _run(sess, p["fd"], sdec)
    steps, bsz, n = res["tok"].shape
    assert (bsz, n) == (BATCH, N) and 1 <= steps <= STEPS
    ref_logits = p["forced_logits"](res["tok"].reshape(steps, bsz * n), N)
    share = _check_against_oracle(res, ref_logits, TEMPERATURE, TOP_K, TOP_P)
    print(parent, "steps", steps, "exact draws", share)
    assert share > 0.95
    for b in range(bsz):                                  # the samples of a sentence differ from each other
        seqs = {tuple(res["tok"][:, b, j]) for j in range(n)}
        assert len(seqs) == n, (b, seqs)
    again = _run(sess, p["fd"], sdec)                     # the same batch again: other salts, other draws
    assert again["salts"] != res["salts"]
    assert again["tok"].shape != res["tok"].shape or not np.array_equal(again["tok"], res["tok"])
    third = _run(sess, p["fd"], sdec)                     # (by now the chunks are replayed graphs: the salt word moved)
    assert third["tok"].shape != again["tok"].shape or not np.array_equal(third["tok"], again["tok"])
    # a session rebuilt with the same seed draws the same
    q = PARENTS[parent](dev)
    sdec2 = _sampler(q["dec"])
    sdec2.keep_logits = True
    rebuilt = _run(q["tfm"].sessions[0], q["fd"], sdec2)
    assert rebuilt["salts"] == res["salts"]
    assert np.array_equal(rebuilt["tok"], res["tok"]) and np.array_equal(rebuilt["lps"], res["lps"])


def test_top_k_1_is_the_greedy_decoder(dev):
    p = _rnn_fast(dev)
    ref = O.decoding_loop(p["params"], O.DecoderSpec(max_output_len=STEPS), O.sentence_encoder(p["params"], p["src"]),
                          None, False)
    live = np.concatenate([np.ones((1, BATCH), bool), ref.mask[:-1]])
    top2 = np.sort(ref.logits, axis=2)[:, :, -2:]
    gap = (top2[:, :, 1] - top2[:, :, 0])[live]
    assert gap.min() > 1e-3, "the fixture has a near-tie ({}): pick another seed".format(gap.min())
    sess = p["tfm"].sessions[0]
    greedy = sess.run(p["dec"].decoded_symbols, p["fd"])
    sdec = _sampler(p["dec"], name="one", num_samples=1, temperature=1.0, top_k=1, top_p=1.0)
    res = _run(sess, p["fd"], sdec)
    assert np.array_equal(res["tok"][:, :, 0], greedy)
    assert np.array_equal(greedy, ref.symbols.astype(np.int32))
    assert (res["kept"][res["tok"] != 0] == 1).all() and (res["lps"] == 0).all()


def test_runner_sentences_and_loss_are_those_of_outputs(dev):
    from neuralmonkey_amd.runners import SamplingRunner
    a, b = _rnn_fast(dev), None
    sdec = _sampler(a["dec"])
    runner = SamplingRunner("target_sample", sdec, sample=2)
    got = a["tfm"].execute(a["ds"], runner.feedables, [runner])[0]
    b = _rnn_fast(dev)                                    # the same seed: the same draws
    res = _run(b["tfm"].sessions[0], b["fd"], _sampler(b["dec"]))
    vocab = b["dec"].vocabulary
    want = vocab.vectors_to_sentences(res["tok"][:, :, 1])
    assert got.outputs["target_sample"] == want
    assert set(got.losses) == {"target_sample/sample_logprob"}
    assert abs(got.losses["target_sample/sample_logprob"] - float(res["lps"][:, 1].mean())) < 1e-5
    assert got.size == BATCH


def test_a_sampling_step_launches_no_torch_kernels(dev):
    from neuralmonkey_amd.runners import SamplingRunner
    from tests.test_no_foreign_kernels_gpu import _foreign_kernels
    p = _rnn_fast(dev)
    runner = SamplingRunner("target_sample", _sampler(p["dec"]))
    foreign = _foreign_kernels(lambda: p["tfm"].execute(p["ds"], runner.feedables, [runner], compute_losses=False))
    assert not foreign, foreign
