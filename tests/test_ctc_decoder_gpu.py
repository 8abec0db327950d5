"""Two whole CTC models on the MI355X, built from INI text (tests/ctc_models.py) and run through CrossEntropyTrainer
and PlainRunner via TensorFlowManager.execute, against a float64 torch restatement of the whole model:

  speech   TemporalFiller(39) -> RecurrentEncoder [(50, bidirectional), (100, forward), (100, backward)] -> CTCDecoder
           (the model of the reference's tests/ctc.ini; features through readers.numpy_reader)
  chars    EmbeddedSequence -> SentenceCNNEncoder -> CTCDecoder, also with the encoder's input dropout on (the engine's
           own mask, regenerated from the same salt and step)

Checked: the summed loss and EVERY variable's gradient of one training step (the restatement's loss is torch's CPU
ctc_loss in float64 on the restated logits, plus the trainer's L2 term), the decoded sentences, train_loss ==
runtime_loss, a checkpoint round trip that restores identical logits, and a short training run whose summed loss falls.
Bounds: the ones smoke() holds a training step to -- 1e-4 relative on the loss, 1e-3 of the largest magnitude on a
gradient."""
import numpy as np
import pytest
import torch

from . import ctc_models as M
from . import ctc_ref as R
from . import sent_cnn_ref as C

pytestmark = pytest.mark.gpu

CELL = ("gates/kernel", "gates/bias", "candidate/kernel", "candidate/bias")


def speech_states(x, lens, p):
    """RecurrentEncoder.temporal_states of the three-layer encoder (recurrent.py:179-217: dynamic_rnn layers that emit
    zeros past the length, a backward layer runs on the length-reversed sequence; final layer norm, eps 1e-6)."""
    cell = lambda scope: {k: p["audio_encoder/{}/OrthoGRUCell/{}".format(scope, k)] for k in CELL}
    fw, _ = C.gru_layer(x, lens, cell("rnn_0_bidirectional/bidirectional_rnn/fw"), False)
    bw, _ = C.gru_layer(x, lens, cell("rnn_0_bidirectional/bidirectional_rnn/bw"), True)
    h, _ = C.gru_layer(torch.cat([fw, bw], 2), lens, cell("rnn_1_forward/rnn"), False)
    h, _ = C.gru_layer(h, lens, cell("rnn_2_backward/rnn"), True)
    h = torch.nn.functional.layer_norm(h, (h.shape[2],), p["audio_encoder/LayerNorm/gamma"],
                                       p["audio_encoder/LayerNorm/beta"], eps=1e-6)
    return h, lens


def chars_states(ids, p, enc, drop):
    mask = (ids != 0).double()
    x = p["char_input/embedding_matrix_0"][ids] * mask[:, :, None]
    local = {n[len(enc.name) + 1:]: v for n, v in p.items() if n.startswith(enc.name + "/")}
    states, _, pmask = C.encoder(x, mask, mask.sum(1).long(), local, enc.filters, enc.segment_size, enc.highway_depth,
                                 drop=drop)
    return states, pmask.sum(1).long()


def reference_step(model, kind, batch, params, drop=None):
    """(summed CTC loss, logits [T, B, K], frame lengths, label lists) in float64; ``params`` require grad."""
    dec = model.runners[0].decoder
    enc = dec.encoder
    if kind == "speech":
        fd = enc.input_sequence.feed_dict(batch)
        feats = [v for k, v in fd.items() if k.name.endswith("/temporal_states")][0]
        lens = [v for k, v in fd.items() if k.name.endswith("/encoder_padding_lengths")][0]
        states, frame_lens = speech_states(torch.tensor(feats, dtype=torch.float64), torch.tensor(lens).long(), params)
    else:
        ids = torch.tensor(enc.input_sequence.feed_dict(batch)[enc.input_sequence.inputs]).long()
        states, frame_lens = chars_states(ids, params, enc, drop)
    logits = (states @ params["decoder/state_to_word_W"] + params["decoder/state_to_word_b"]).transpose(0, 1)
    labels = R.prepare_labels(dec.feed_dict(batch, train=True)[dec.train_tokens], dec.merge_repeated_targets)
    flat = torch.tensor([c for lab in labels for c in lab], dtype=torch.long)
    loss = torch.nn.functional.ctc_loss(torch.log_softmax(logits, -1), flat, frame_lens,
                                        torch.tensor([len(lab) for lab in labels]), blank=logits.shape[2] - 1,
                                        reduction="sum", zero_infinity=True)
    return loss, logits, frame_lens, labels


def snapshot(store):
    return {n: store[n].detach().double().cpu().requires_grad_(True) for n in store.names()}


def fetch_logits(model, batch, feedables):
    from neuralmonkey_amd.runtime import RunContext
    fd = {}
    for part in feedables:
        fd.update(part.feed_dict(batch, train=False))
    dec = model.runners[0].decoder
    out = dec.logits(RunContext(model.tf_manager.sessions[0], fd)).clone()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kind,keep", [("speech", 1.0), ("chars", 1.0), ("chars", 0.5)])
def test_training_step_decoding_and_checkpoint_against_float64(dev, tmp_path, kind, keep):
    from neuralmonkey_amd import ops
    from neuralmonkey_amd.runtime import RunContext
    model, targets = M.load(tmp_path, kind, dev, keep=keep)
    tfm, trainer, runner = model.tf_manager, model.trainers[0], model.runners[0]
    dec = runner.decoder
    sess = tfm.sessions[0]
    store = sess.store
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    batch = next(iter(model.train_dataset.batches()))
    assert len(batch) == 8
    # variables moved off their initial values a little (no bias at exactly zero, no gate at its initial value)
    g = torch.Generator(device=dev).manual_seed(7)
    for n in store.names():
        store[n].add_(torch.randn(store[n].shape, device=dev, generator=g) * 0.05)
        if n.endswith("/bias_H"):
            # a highway layer's relu branch is dead at its initial bias of -1 on these small inputs: weight_H and bias_H
            # would be compared on gradients that are exactly zero.  Shifted so that the branch is live.
            store[n].add_(1.0)

    drop = None
    if keep < 1.0:                                       # the mask the step below draws: same salt, same step counter
        enc = dec.encoder
        ids = enc.input_sequence.feed_dict(batch)[enc.input_sequence.inputs]
        ones = torch.ones(ids.shape[0] * ids.shape[1], enc.input_sequence.dimension, device=dev)
        mask = torch.empty_like(ones)
        ops.dropout(ones, mask, keep, RunContext(sess, {}).salt(enc.name, "cnn_input"), step=sess.step_tensor())
        drop = mask.double().cpu().view(ids.shape[0], ids.shape[1], -1)
        assert 0.3 < float((drop == 0).double().mean()) < 0.7

    # ---- one training step: loss and every variable's gradient
    params = snapshot(store)
    loss, _, frame_lens, labels = reference_step(model, kind, batch, params, drop)
    reg = sum((params[n] ** 2).sum() for n in trainer.regularizable(store))
    (loss + trainer.l2_weight * reg).backward()
    res = tfm.execute(batch, feedables, [trainer], train=True)[0]
    got_loss = float(res.losses["decoder - cost"])
    print("{} keep {}: loss {:.6f} (float64 {:.6f})".format(kind, keep, got_loss, float(loss)))
    assert abs(got_loss - float(loss)) < 1e-4 * float(loss), (got_loss, float(loss))
    assert [len(l) for l in labels] == [len(t) for t in targets] and 0 in [len(l) for l in labels]
    worst = 0.0
    for n, p in params.items():
        want = p.grad if p.grad is not None else torch.zeros_like(p)
        err = float((store.g(n).double().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-6)
        worst = max(worst, err)
        assert err < 1e-3, (n, err)
        assert float(want.abs().max()) > 0 or "embedding" in n, n          # every variable is reached by the loss
    print("{} keep {}: {} variables, worst gradient error {:.3g} of its largest magnitude".format(kind, keep, len(params),
                                                                                              worst))

    # ---- decoding through PlainRunner (inference mode: no dropout), on the updated variables
    out = tfm.execute(batch, feedables, [runner])[0]
    params = snapshot(store)
    with torch.no_grad():
        loss_after, logits, frame_lens, _ = reference_step(model, kind, batch, params, None)
    have = fetch_logits(model, batch, feedables)
    assert tuple(have.shape) == tuple(logits.shape)                          # time-major [T, B, V + 1]
    bound = 1e-4 * float(logits.abs().max())
    assert float((have.double().cpu() - logits).abs().max()) < bound
    sure = R.top_two_gap(logits.numpy()) > 2 * bound
    assert (~sure).mean() <= 0.01
    _, want = R.greedy(logits.numpy(), frame_lens.numpy(), dec.merge_repeated_outputs)
    sentences = out.outputs["target"]
    assert len(sentences) == len(batch)
    for b, sent in enumerate(sentences):
        if sure[:int(frame_lens[b]), b].all():
            assert sent == [dec.vocabulary.index_to_word[c] for c in want[b]], b
    train_loss, runtime_loss = out.losses["target/train_loss"], out.losses["target/runtime_loss"]
    assert train_loss == runtime_loss and abs(train_loss - float(loss_after)) < 1e-4 * float(loss_after)

    # ---- checkpoint round trip: identical logits
    path = str(tmp_path / "variables.data")
    tfm.save(path)
    kept = {n: store[n].clone() for n in store.names()}
    for n in store.names():
        store[n].mul_(0.5)
    sess.variables_changed()
    assert not torch.equal(fetch_logits(model, batch, feedables), have)
    tfm.restore(path)
    assert all(torch.equal(store[n], kept[n]) for n in store.names())
    assert torch.equal(fetch_logits(model, batch, feedables), have)


def test_ragged_features_and_a_batch_that_emits_nothing(dev, tmp_path):
    """Feature sequences of different lengths in one batch (TemporalFiller pads, the mask gives the frame lengths):
    loss against float64; and a decoder whose blank wins everywhere decodes to empty sentences."""
    from neuralmonkey_amd.dataset import Dataset
    model, _ = M.load(tmp_path, "speech", dev)
    tfm, trainer, runner = model.tf_manager, model.trainers[0], model.runners[0]
    store = tfm.sessions[0].store
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    rng = np.random.default_rng(3)
    feats = [rng.standard_normal((n, 39)).astype(np.float32) for n in (17, 5, 1, 9, 2)]
    words = [["yes", "no"], ["no", "no", "maybe"], ["yes"], [], ["yes", "yes", "yes"]]   # the last: 3 labels, 2 frames
    batch = Dataset("ragged", series={"source": feats, "target": words})
    params = snapshot(store)
    with torch.no_grad():
        loss, _, frame_lens, labels = reference_step(model, "speech", batch, params)
    assert frame_lens.tolist() == [17, 5, 1, 9, 2] and not R.has_alignment(labels[4], 2, True)
    out = tfm.execute(batch, feedables, [runner])[0]
    assert abs(out.losses["target/train_loss"] - float(loss)) < 1e-4 * float(loss)
    assert all(len(s) <= n for s, n in zip(out.outputs["target"], frame_lens.tolist()))
    store["decoder/state_to_word_b"][-1] = 100.0                      # the blank wins every frame
    tfm.sessions[0].variables_changed()
    out = tfm.execute(batch, feedables, [runner])[0]
    assert out.outputs["target"] == [[] for _ in words]


def test_thirty_adam_steps_lower_the_summed_loss(dev, tmp_path):
    model, _ = M.load(tmp_path, "speech", dev, lr=0.01)
    tfm, trainer = model.tf_manager, model.trainers[0]
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    batch = next(iter(model.train_dataset.batches()))
    losses = [float(tfm.execute(batch, feedables, [trainer], train=True)[0].losses["decoder - cost"]) for _ in range(30)]
    print("summed CTC loss, 30 Adam steps: {:.3f} -> {:.3f}".format(losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
