"""Whole beam searches with 17 to 64 hypotheses on tiny models: RNN decoder with Bahdanau attention, Transformer
decoder through the key/value cache, an ensemble of two RNN models, and the runner's rank selection.

Near-ties are common in a wide beam (65 neighbouring scores per sentence and step), so the oracle is made to FOLLOW the
engine's ``selection_history`` and every selection of every step is accounted for with
tests/beam_accounting.py:account_for_every_selection (near-tie margin 1e-5, that module's own): each (step, sentence)
top-k list is the oracle's own or a legitimate ordering of a near-tie, and the end states, lengths and flags agree
for all sentences.  The Transformer's follow mode is oracle/ensemble_ref.py:beam_ensemble_transformer over ONE
oracle/transformer_ref.py model (an ensemble of one model is the plain search, tests/test_reference_exec.py); the
free-running ``TransformerModel.beam`` is compared as tests/test_transformer_gpu.py does it, in the sentences whose own
reported gap exceeds 1e-5 (at beam 24 all four sentences for the chosen seed; at beam 64 some two of the 65
neighbours lie closer than that in every sentence of every seed tried on the CPU, which is why the follow mode is
the check there).

The last tests show that beams of 16 and 5 still go through the narrow kernels: ``ops.beam_topk_step_wide`` is
not reached."""
import numpy as np
import pytest

from oracle import ensemble_ref as E
from oracle import general_ref as G
from oracle import nm_oracle as O
from oracle import transformer_ref as TRF

from .beam_accounting import account_for_every_selection
from .test_engine_gpu import _ids_to_words, _setup
from .test_ensemble_gpu import _batch, _model, _params, _sentences
from .test_transformer_gpu import CASES, _build, _data

pytestmark = pytest.mark.gpu
NEAR_TIE = 1e-5


def _np(x):
    return np.asarray(x.cpu() if hasattr(x, "cpu") else x)


def _count_wide_calls(monkeypatch):
    from neuralmonkey_amd import ops
    calls, real = [], ops.beam_topk_step_wide

    def counted(*a, **kw):
        calls.append(kw.keys())
        return real(*a, **kw)
    monkeypatch.setattr(ops, "beam_topk_step_wide", counted)
    return calls


def _rnn_search(dev, vocab, emb, rnn, batch, slen, tlen, beam, alpha):
    model, params, ds, src, _ = _setup(dev, vocab, emb, rnn, batch, slen, tlen, True, beam=beam, max_steps=tlen,
                                       length_normalization=alpha)
    enc = O.sentence_encoder(params, src)
    spec = O.DecoderSpec(max_output_len=max(slen, tlen))
    sess = model.tf_manager.sessions[0]
    fd = {}
    for f in model.beam_runner.feedables:
        fd.update(f.feed_dict(ds, train=False))
    got = sess.run({"bs": model.beam_decoder.outputs, "sel": model.beam_decoder.selection_history}, fd)
    sel_beam, sel_word = (_np(x) for x in got["sel"])
    tok = np.asarray(got["bs"].last_search_step_output.token_ids)
    ref = O.beam_search(params, spec, enc, beam, tlen, alpha, follow=(sel_beam, sel_word))
    return dict(model=model, params=params, ds=ds, enc=enc, spec=spec, out=got["bs"], tok=tok, ref=ref,
                sel=(sel_beam, sel_word))


@pytest.mark.parametrize("vocab,emb,rnn,batch,slen,tlen,beam,alpha", [
    (300, 16, 16, 3, 9, 8, 17, 1.0),
    (500, 32, 32, 6, 20, 12, 32, 0.6),
    (500, 32, 32, 2, 12, 10, 64, 0.0),
    (300, 16, 16, 1, 9, 8, 20, 0.6),      # the reference's own (batch-1) regime
])
def test_rnn_wide_beam_every_selection_is_accounted_for(dev, monkeypatch, vocab, emb, rnn, batch, slen, tlen, beam,
                                                         alpha):
    calls = _count_wide_calls(monkeypatch)
    w = _rnn_search(dev, vocab, emb, rnn, batch, slen, tlen, beam, alpha)
    assert calls, "a beam of {} did not reach the wide kernel".format(beam)
    sel_beam, sel_word = w["sel"]
    assert w["tok"].shape == w["ref"].token_ids.shape and w["tok"].shape[1:] == (batch, beam)
    assert sel_beam.shape[1:] == (batch, beam) and sel_beam.min() >= 0 and sel_beam.max() < beam
    exact, reordered, never = account_for_every_selection(w["ref"], sel_beam, sel_word, w["tok"], w["out"], beam, vocab,
                                                          NEAR_TIE)
    print("RNN beam-{}: {:.2%} of the (step, sentence) lists exactly the oracle's, {} a legitimate ordering of a "
          "near-tie; {:.0%} of the sentences never met one".format(beam, exact, reordered, never))


@pytest.mark.parametrize("beam,seed", [(24, 9), (64, 9)])
def test_transformer_wide_beam_every_selection_is_accounted_for(dev, monkeypatch, beam, seed):
    calls = _count_wide_calls(monkeypatch)
    cfg, d, ff = CASES["wide"]
    vocab, steps, batch = 100, 8, 4
    m = _build(dev, cfg, d, ff, max_len=steps, beam=beam, seed=seed, vocab_size=vocab)
    ds, src, _ = _data(batch, 7, 6, steps, with_target=False, vocab_size=vocab)
    sess = m["tfm"].sessions[0]
    fd = {}
    for part in (m["enc"].input_sequence, m["enc"], m["dec"]):
        fd.update(part.feed_dict(ds, train=False))
    got = sess.run({"bs": m["bdec"].outputs, "sel": m["bdec"].selection_history}, fd)
    assert calls
    out = got["bs"]
    sel_beam, sel_word = (_np(x) for x in got["sel"])
    tok = np.asarray(out.last_search_step_output.token_ids)
    model = TRF.TransformerModel(m["params"], cfg)
    ref = E.beam_ensemble_transformer([model], src, beam, steps, 0.6, follow=(sel_beam, sel_word))
    assert tok.shape == ref.token_ids.shape == (steps + 1, batch, beam)
    exact, reordered, never = account_for_every_selection(ref, sel_beam, sel_word, tok, out, beam, vocab, NEAR_TIE)
    # ... and the free-running oracle of tests/test_transformer_gpu.py, in the sentences it decides by more than 1e-5
    free_tok, free_scores, _ = model.beam(src, beam, steps, 0.6)
    decided = np.min(np.stack(model.beam_gaps), axis=0) > NEAR_TIE
    share = float(decided.mean())
    print("Transformer beam-{}: {:.2%} of the lists exact, {} re-ordered near-ties; free-running oracle compared in "
          "{:.0%} of the sentences".format(beam, exact, reordered, share))
    if beam == 24:
        assert share >= 0.5
    assert np.array_equal(tok[1:, decided], free_tok[1:, decided])
    if decided.any():
        sc = np.asarray(out.last_search_step_output.scores)[decided]
        assert np.abs(sc - free_scores[decided]).max() <= 1e-4 * np.abs(free_scores[decided]).max()


def test_ensemble_of_two_rnn_models_with_a_beam_of_20(dev, monkeypatch):
    calls = _count_wide_calls(monkeypatch)
    beam = 20
    model = _model(dev, 2, beam=beam)
    p0, p1 = _params(37), _params(38)
    for sess, p in zip(model.tf_manager.sessions, (p0, p1)):
        sess.store.load_state_dict(p)
    ds, src = _batch(7)
    cfg = G.Config(rnn_layers=((16, "bidirectional", "GRU"),), rnn_size=16)
    to32 = lambda p: {k: np.asarray(v, np.float32) for k, v in p.items()}
    tok, scores, gap = E.beam_ensemble([G.GeneralModel(to32(p0), cfg), G.GeneralModel(to32(p1), cfg)], src, beam, 10,
                                       0.6)
    assert gap > NEAR_TIE                                   # the seeds were chosen on the CPU for this
    res = model.tf_manager.execute(ds, model.beam_runner.feedables, [model.beam_runner], compute_losses=False)[0]
    assert calls and all("rmax_in" in kw for kw in calls)   # the ensemble convention: given (zero) statistics
    w2i = model.tgt_vocab._word_to_index                    # pylint: disable=protected-access
    assert [[w2i[w] for w in sent] for sent in res.outputs["target_beam"]] == _sentences(tok)
    want = float(np.mean(scores[:, 0]) * len(scores))
    assert abs(res.losses["target_beam/beam_search_score"] - want) <= 1e-4 * abs(want)


def test_runner_returns_hypothesis_17_of_a_beam_of_20(dev):
    from neuralmonkey_amd.runners import BeamSearchRunner
    vocab, batch, tlen, beam, rank, alpha = 300, 5, 8, 20, 17, 0.6
    w = _rnn_search(dev, vocab, 16, 16, batch, 9, tlen, beam, alpha)
    model, ref = w["model"], w["ref"]
    sel_beam, sel_word = w["sel"]
    account_for_every_selection(ref, sel_beam, sel_word, w["tok"], w["out"], beam, vocab, NEAR_TIE)
    runner = BeamSearchRunner("target_beam17", model.beam_decoder, rank=rank)
    res = model.tf_manager.execute(w["ds"], runner.feedables, [runner])[0]
    # sentences that never met a near-tie: the free-running oracle makes the engine's selections there
    f = ref.follow
    steps = f["own_idx"].shape[0]
    given = sel_beam[:steps].astype(np.int64) * vocab + sel_word[:steps].astype(np.int64)
    clear = (f["own_idx"][:, :, :beam] == given).all(-1).all(0)
    free = O.beam_search(w["params"], w["spec"], w["enc"], beam, tlen, alpha)
    want, _ = O.beam_tokens(free, rank)
    want = _ids_to_words(model.tgt_vocab, want)
    print("rank {} of {}: {} of {} sentences without a near-tie".format(rank, beam, int(clear.sum()), batch))
    assert clear.any()
    for s in np.nonzero(clear)[0]:
        assert res.outputs["target_beam17"][s] == want[s], s
    loss = float(np.mean(ref.scores[:, rank - 1]) * batch)
    assert abs(res.losses["target_beam17/beam_search_score"] - loss) <= 1e-3 * abs(loss)


@pytest.mark.parametrize("beam", [16, 5])
def test_narrow_beams_do_not_reach_the_wide_kernel(dev, monkeypatch, beam):
    calls = _count_wide_calls(monkeypatch)
    w = _rnn_search(dev, 300, 16, 16, 3, 9, 8, beam, 0.6)
    sel_beam, sel_word = w["sel"]
    account_for_every_selection(w["ref"], sel_beam, sel_word, w["tok"], w["out"], beam, 300, NEAR_TIE)
    cfg, d, ff = CASES["wide"]
    m = _build(dev, cfg, d, ff, max_len=8, beam=beam, vocab_size=100)
    ds, _, _ = _data(4, 7, 6, 8, with_target=False, vocab_size=100)
    fd = {}
    for part in (m["enc"].input_sequence, m["enc"], m["dec"]):
        fd.update(part.feed_dict(ds, train=False))
    got = m["tfm"].sessions[0].run(m["bdec"].outputs, fd)
    assert np.asarray(got.last_search_step_output.token_ids).shape[1:] == (4, beam)
    assert calls == []
