"""WordAlignmentDecoder / WordAlignmentRunner on the MI355X.

  * a synthetic translation model (synthetic.build_translation_model: embeddings 8, RNN 8, max_len 6, vocabularies of
    40, batch 4, ragged lengths) with an alignment objective of weight 0.5 beside the cost objective: both losses and
    every variable's gradient against the float64 restatement of the WHOLE step -- oracle/general_ref.py for the
    translation model, tests/align_ref.py (TensorFlow's registered gradient) on its attention weights -- on the
    hand-scheduled path (no dropout) and on the tape (``dropout_keep_prob=0.5`` on the decoder, the step's masks replayed
    from their salts as tests/test_general_gpu.py replays them).  Tolerances of the neighbouring model tests: 1e-4
    relative on a loss, 1e-3 of a tensor's largest magnitude on its gradient;
  * weight 0: parent loss and gradient bit-equal to a trainer without the alignment objective (hand-scheduled path),
    but for the two embedding tables, whose atomically summed gradients differ from run to run without any objective;
  * the captured step graph gives the eager step's losses and gradient;
  * an alignment-only trainer: the vocabulary and output projections get exact zeros, the rest the oracle's gradient;
  * runtime: the runner's [B, S, T] is the recorded weights transposed, ``decoded`` their softmax, ``runtime_loss`` 0;
  * tests/alignment.ini (with ``maxout_size=9``, see tests/test_alignment_host.py) trains three optimizer steps."""
import numpy as np
import pytest
import torch

from oracle import general_ref as G
from oracle import nm_oracle as O

from . import align_ref as R
from .test_alignment_host import ref_root, with_matching_maxout  # noqa: F401  pylint: disable=unused-import

pytestmark = pytest.mark.gpu

VOCAB, MAX_LEN, BATCH = 40, 6, 4


def build(dev, keep=1.0, weights=(1.0, 0.5), objectives="both", src_emb=8):
    """The model, its trainer and its alignment parts; ``objectives``: both | parent | alignment.  ``src_emb``: a source
    embedding size that is no multiple of 4 sends the encoder to the tape as well (a step can then be captured)."""
    from neuralmonkey_amd import synthetic
    from neuralmonkey_amd.decoders import WordAlignmentDecoder
    from neuralmonkey_amd.runners import WordAlignmentRunner
    from neuralmonkey_amd.trainers import CrossEntropyTrainer
    m = synthetic.build_translation_model(vocab_src=VOCAB, vocab_tgt=VOCAB, emb=src_emb, dec_emb=8, rnn=8, max_len=MAX_LEN, beam_size=0,
                                          with_trainer=False, device=str(dev), seed=5)
    dec = m.decoder
    if keep != 1.0:                       # (the builder has no such argument: set before anything reads it)
        dec.dropout_keep_prob = keep
        dec.__dict__.pop("_enc_proj_cached", None)
    wad = WordAlignmentDecoder(m.encoder, dec, "ali", "aligner")
    decoders = {"both": [dec, wad], "parent": [dec], "alignment": [wad]}[objectives]
    trainer = CrossEntropyTrainer(decoders=decoders, decoder_weights=list(weights)[:len(decoders)], l2_weight=0.0,
                                  clip_norm=None)
    store = m.tf_manager.sessions[0].store
    rng = np.random.default_rng(5)
    vals = store.state_dict()
    for name, v in vals.items():          # non-degenerate weights (tests/test_general_gpu.py)
        if v.ndim >= 2 or name.endswith("attn_similarity_v"):
            vals[name] = (rng.standard_normal(v.shape) * 0.35).astype(np.float32)
        elif "bias" in name or name.endswith("_b"):
            vals[name] = (v + rng.standard_normal(v.shape) * 0.1).astype(np.float32)
    store.load_state_dict(vals)
    runner = WordAlignmentRunner("alignment", m.attention, dec)
    return dict(m=m, dec=dec, wad=wad, trainer=trainer, tfm=m.tf_manager, store=store, params=store.state_dict(),
                runner=runner, keep=keep)


def data(seed=3):
    """(dataset with an ``ali`` series, padded source ids [B, S], target ids [T, B], fed alignment [B, 6, 6])."""
    from neuralmonkey_amd import synthetic
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    src, tgt = synthetic.synthetic_ids(seed, BATCH, MAX_LEN, MAX_LEN, VOCAB, ragged=True)
    rng = np.random.default_rng(seed)
    ali = []
    for b in range(BATCH):
        mat = (rng.random((MAX_LEN, MAX_LEN)) * (rng.random((MAX_LEN, MAX_LEN)) < 0.5)).astype(np.float32)
        for t in range(MAX_LEN):
            kind = (b + t) % 3
            if kind == 0 and mat[t].sum() > 0:
                mat[t] /= mat[t].sum()                               # a normalised row
            elif kind == 1:
                mat[t] = 0.0                                         # an unaligned target word
        ali.append(mat)                                              # (kind 2: as ``normalize=False`` leaves it)
    ds = Dataset("synthetic", {"source": src, "target": tgt, "ali": ali}, BatchingScheme(batch_size=BATCH))
    src_ids = O.pad_ids([list(s) for s in src], MAX_LEN)
    tgt_tb = np.ascontiguousarray(O.pad_ids([list(s) for s in tgt], MAX_LEN, add_end_symbol=True).T)
    return ds, src_ids, tgt_tb, np.stack(ali)


def oracle_step(params, keep, src, tgt, ali, w_parent, w_align):
    """float64: (parent loss, alignment loss, {variable: gradient of w_parent * parent + w_align * alignment})."""
    cfg = G.Config(enc_name="encoder", dec_name="decoder", att_name="attention", rnn_layers=((8, "bidirectional", "GRU"),),
                   rnn_size=8, dec_dropout=keep, include_final_layer_norm="encoder/LayerNorm/gamma" in params)
    ref = G.GeneralModel(params, cfg, dtype=torch.float64, requires_grad=True)
    xent, _, weights = ref.train_loss(src, tgt, train=True)
    assert tuple(weights.shape) == (tgt.shape[0], tgt.shape[1], src.shape[1])
    align = R.train_loss(weights, ali, (tgt != 0).astype(np.float64))
    names = list(ref.p)
    grads = torch.autograd.grad(w_parent * xent + w_align * align, [ref.p[n] for n in names], allow_unused=True)
    return float(xent.detach()), float(align.detach()), {
        n: (np.zeros(tuple(ref.p[n].shape)) if g is None else g.numpy()) for n, g in zip(names, grads)}


def compare_gradients(store, want, skip=()):
    bad = {}
    for name in store.names():
        got = store.g(name).cpu().numpy().astype(np.float64).reshape(-1)
        ref = want[name].reshape(-1)
        if name.endswith("attn_bias"):       # identically zero (softmax shift invariance), here too
            assert abs(got[0]) < 1e-5 and abs(ref[0]) < 1e-5
            continue
        err = float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6))
        if err > 1e-3 and name not in skip:
            bad[name] = err
    assert not bad, "gradient mismatch: {}".format(bad)


def train_once(model, ds):
    return model["tfm"].execute(ds, model["trainer"].feedables, [model["trainer"]], train=True)[0]


@pytest.mark.parametrize("keep", [1.0, 0.5], ids=["hand_scheduled", "taped"])
def test_alignment_objective_beside_the_cost_objective(dev, keep):
    model = build(dev, keep)
    assert model["dec"].uses_general_path(True) == (keep != 1.0)
    ds, src, tgt, ali = data()
    want_parent, want_align, want = oracle_step(model["params"], keep, src, tgt, ali, 1.0, 0.5)
    res = train_once(model, ds)
    print("parent {} / {}, alignment {} / {}".format(res.losses["decoder - cost"], want_parent,
                                                     res.losses["aligner - cost"], want_align))
    assert abs(res.losses["decoder - cost"] - want_parent) <= 1e-4 * abs(want_parent)
    assert abs(res.losses["aligner - cost"] - want_align) <= 1e-4 * abs(want_align)
    assert want_align > 1.0                                            # a sum over the batch, not a mean
    compare_gradients(model["store"], want)
    # and the term matters: the parent's gradient alone is somewhere else
    _, _, parent_only = oracle_step(model["params"], keep, src, tgt, ali, 1.0, 0.0)
    name = "attention/attn_key_projection"
    assert np.abs(parent_only[name] - want[name]).max() > 1e-2 * np.abs(want[name]).max()


def test_weight_zero_is_bit_equal_to_no_alignment_objective(dev):
    """The parent's loss and every gradient the step computes reproducibly are BIT-equal.  The two embedding tables'
    gradients are summed by ``nm_embedding_scatter_add`` with float atomics, in whatever order the rows arrive: two
    runs of the trainer WITHOUT the objective already differ there (measured: 9.3e-10 in ``decoder/word_embeddings``,
    one unit in the last place of an entry, in three of four repeats), so for those two tensors the comparison is the
    reordering bound of a sum of at most T * B addends instead: (T * B - 1) float32 epsilons of the largest entry."""
    ds, _, tgt, _ = data()
    with_term = build(dev, 1.0, weights=(1.0, 0.0))
    res = train_once(with_term, ds)
    store = with_term["store"]
    grads = {n: store.g(n).clone() for n in store.names()}
    loss = res.losses["decoder - cost"]
    assert np.isfinite(res.losses["aligner - cost"]) and res.losses["aligner - cost"] > 0
    without = build(dev, 1.0, objectives="parent")
    res = train_once(without, ds)
    assert res.losses["decoder - cost"] == loss
    atomic = [n for n in grads if "embedding" in n]
    assert sorted(atomic) == ["decoder/word_embeddings", "encoder_input/embedding_matrix_0"]
    for name, got in grads.items():
        want = without["store"].g(name)
        if name in atomic:
            bound = (tgt.size - 1) * float(np.finfo(np.float32).eps) * float(want.abs().max())
            assert float((got - want).abs().max()) <= bound, name
        else:
            assert torch.equal(got, want), name


def test_alignment_only_trainer(dev):
    model = build(dev, 1.0, weights=(1.0,), objectives="alignment")
    ds, src, tgt, ali = data()
    _, want_align, want = oracle_step(model["params"], 1.0, src, tgt, ali, 0.0, 1.0)
    res = train_once(model, ds)
    assert set(res.losses) == {"aligner - cost", "L1", "L2"}
    assert abs(res.losses["aligner - cost"] - want_align) <= 1e-4 * abs(want_align)
    store = model["store"]
    above = [n for n in store.names() if n.startswith("decoder/state_to_word") or "/dense/" in n]
    assert len(above) == 4, above
    for name in store.names():
        got = store.g(name).cpu().numpy()
        if name in above:                 # nothing above the attention: the cross entropy's scale is zero
            assert not got.any() and not want[name].any(), name
        elif not name.endswith("attn_bias"):
            assert np.abs(got).max() > 0, name
    compare_gradients(store, want)


def _steps(dev, graphs, keep, visits=4):
    model = build(dev, keep, src_emb=6)
    assert model["wad"].graph_safe_training(True)
    sess = model["tfm"].sessions[0]
    sess.use_step_graphs = graphs
    ds, _, _, _ = data()
    losses = []
    for _ in range(visits):
        res = train_once(model, ds)
        losses.append([res.losses["decoder - cost"], res.losses["aligner - cost"]])
    replayed = sum(1 for st in sess.__dict__.get("_step_graphs", {}).values() if st[0] == 2)
    return np.asarray(losses), model["store"].ensure_grad().cpu().numpy(), replayed


def test_captured_step_equals_the_eager_one(dev):
    l_eager, g_eager, n_eager = _steps(dev, False, 0.5)
    l_graph, g_graph, n_graph = _steps(dev, True, 0.5)
    assert n_eager == 0
    assert n_graph >= 1, "no training step was captured: graph_safe_training refused this model"
    assert np.isfinite(l_graph).all() and np.unique(np.round(l_graph[:, 1], 5)).size == len(l_graph)
    assert np.abs(l_graph - l_eager).max() <= 1e-5 * np.abs(l_eager).max(), (l_eager, l_graph)
    assert np.abs(g_graph - g_eager).max() <= 1e-5 * np.abs(g_eager).max()


def test_runtime_alignment_and_decoded(dev):
    model = build(dev, 1.0)
    ds, src, _, _ = data()
    m, wad, runner = model["m"], model["wad"], model["runner"]
    out = model["tfm"].execute(ds, m.greedy_runner.feedables | runner.feedables, [m.greedy_runner, runner])
    alignment = np.asarray(out[1].outputs["alignment"])
    assert out[1].losses == {} and alignment.ndim == 3
    recorded = m.attention.histories["decoder_run"].cpu().numpy()           # [T, B, S] of that run
    steps, bsz, slen = recorded.shape
    assert (bsz, slen) == (BATCH, src.shape[1]) and 1 <= steps <= MAX_LEN
    assert alignment.shape == (bsz, slen, steps) and np.array_equal(alignment, np.transpose(recorded, (1, 2, 0)))
    assert np.abs(recorded.sum(axis=2) - 1.0).max() < 1e-5
    fd = {}
    for part in m.greedy_runner.feedables | runner.feedables | {wad}:
        fd.update(part.feed_dict(ds, train=False))
    seen = model["tfm"].sessions[0].run({"decoded": wad.decoded, "loss": wad.runtime_loss, "alignment": runner.alignment},
                                        fd)
    assert seen["loss"] == 0
    decoded, weights = np.asarray(seen["decoded"]), np.transpose(np.asarray(seen["alignment"]), (2, 0, 1))
    want = R.rows(weights, np.zeros((bsz, steps, slen), np.float32), np.ones((steps, bsz)))["decoded"]
    assert decoded.shape == (bsz, steps, slen)
    assert np.abs(decoded - want).max() <= 1e-4 * np.abs(want).max()
    # without a trainer the train loss is that of the teacher-forced pass's own weights
    fd = {}
    for part in model["trainer"].feedables:
        fd.update(part.feed_dict(ds, train=False))
    seen = model["tfm"].sessions[0].run({"loss": wad.train_loss, "xents": wad.train_xents}, fd)
    _, _, tgt, ali = data()
    recorded = m.attention.histories["decoder_train"].cpu().numpy()
    want = R.rows(recorded, ali, (tgt != 0).astype(np.float64))
    assert abs(float(seen["loss"]) - want["loss"]) <= 1e-4 * want["loss"]
    assert np.abs(np.asarray(seen["xents"]) - want["loss_rows"]).max() <= 1e-4 * np.abs(want["loss_rows"]).max()


def test_alignment_ini_trains(dev, ref_root):  # noqa: F811
    from neuralmonkey_amd.dataset import BatchingScheme
    from .test_reference_inis import load_verbatim
    model = load_verbatim(ref_root, with_matching_maxout(ref_root), device=str(dev))
    trainer, tfm = model.trainers[0], model.tf_manager
    dec, wad = [o.decoder for o in trainer.objectives]
    store = tfm.sessions[0].store
    before = store.state_dict()
    losses = []
    for i, batch in zip(range(3), model.train_dataset.batches(BatchingScheme(batch_size=16))):
        res = tfm.execute(batch, trainer.feedables, [trainer], train=True)[0]
        losses.append([res.losses["bahdanau_decoder - cost"], res.losses["alignment_decoder - cost"]])
        if i == 0:
            weights = wad.attention.histories["bahdanau_decoder_train"].cpu().numpy()
            ali = wad.feed_dict(batch, train=True)[wad.ref_alignment]
            ids = dec.feed_dict(batch, train=True)[dec.train_tokens]               # [B, T]
            assert ali.shape == (16, 8, 12) and weights.shape[1] == 16 and weights.shape[0] == ids.shape[1]
            want = R.rows(weights, ali, (ids.T != 0).astype(np.float64))["loss"]
            assert abs(losses[0][1] - want) <= 1e-4 * want, (losses[0][1], want)
    assert tfm.sessions[0].global_step == 3 and np.isfinite(losses).all() and (np.asarray(losses) > 0).all()
    after = store.state_dict()
    moved = [n for n in before if not np.array_equal(before[n], after[n])]
    assert len(moved) >= len(before) - 1, sorted(set(before) - set(moved))        # (attn_bias: gradient identically zero)
    out = tfm.execute(model.val_dataset, model.runners[0].feedables, model.runners)
    assert len(out[0].outputs["target"]) == len(model.val_dataset)
