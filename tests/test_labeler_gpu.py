"""SequenceLabeler / EmbeddingsLabeler / LabelRunner on the MI355X.

  * every fixture of tests/golden/labeler (numbers of the REFERENCE'S OWN Python, see make_labeler_golden.py): the
    fixture's variables loaded by name, its strings fed; logits, log-probabilities, xents and cost within 1e-4 of the
    tensor's largest magnitude (``close`` of tests/test_reference_exec_gpu.py), decoded ids and the runner's sentences
    equal;
  * the engine's gradient against central differences of the reference's cost (the bounds of
    test_engine_gradients_against_the_reference_finite_differences);
  * head + encoder states as a leaf against torch autograd in float64: every head variable's gradient and d states by
    the unit method (unit = float32 evaluation of tests/label_ref.py against its float64 evaluation, 16 units, capped
    by smoke()'s 1e-4 relative on the loss and 1e-3 of the largest magnitude on a gradient);
  * the reference's tests/labeler.ini and tests/bert.ini from the committed archive: 30 training steps, the runners;
  * a captured training step equals the eager one; no step launches a kernel of the tensor library."""
import json
import os

import numpy as np
import pytest
import torch

from . import label_ref as R
from . import labeler_models as M
from .test_labeler_host import FIX, FORWARD_CASES, ref_root  # noqa: F401  pylint: disable=unused-import
from .test_reference_exec_gpu import close, load_variables, unpad, vocabulary

pytestmark = pytest.mark.gpu

MULTIPLE = 16.0
EPS32 = float(np.finfo(np.float32).eps)


def load(case):
    z = np.load(os.path.join(FIX, case + ".npz"))
    return z, json.loads(str(z["cfg"])), {k[2:]: z[k] for k in z.files if k.startswith("p/")}


def build(dev, cfg):
    from neuralmonkey_amd import tf_shim
    from neuralmonkey_amd.decoders import EmbeddingsLabeler, SequenceLabeler
    from neuralmonkey_amd.encoders import RecurrentEncoder
    from neuralmonkey_amd.encoders.transformer import TransformerEncoder
    from neuralmonkey_amd.model.sequence import EmbeddedSequence
    from neuralmonkey_amd.runners import LabelRunner, XentRunner
    from neuralmonkey_amd.runtime import reset_registry
    from neuralmonkey_amd.tf_manager import TensorFlowManager
    from neuralmonkey_amd.trainers import CrossEntropyTrainer
    reset_registry()
    sv, tv = vocabulary(cfg["src_vocab"]), vocabulary(cfg["tag_vocab"])
    seq = EmbeddedSequence(name="encoder_input", vocabulary=sv, data_id="source", embedding_size=cfg["emb"])
    if cfg["encoder"] == "gru":
        enc = RecurrentEncoder(name="encoder", input_sequence=seq, rnn_layers=[(cfg["rnn"], "bidirectional", "GRU")])
    else:
        enc = TransformerEncoder(name="encoder", input_sequence=seq, ff_hidden_size=cfg["ff"], depth=cfg["depth"],
                                 n_heads=cfg["heads"])
    encoders, feedables = [enc], [seq, enc]
    if cfg["second_encoder"] is not None:
        enc2 = RecurrentEncoder(name="encoder2", input_sequence=seq,
                                rnn_layers=[(cfg["second_encoder"], "forward", "GRU")])
        encoders.append(enc2)
        feedables.append(enc2)
    act = {"relu": tf_shim.nn.relu, "tanh": tf_shim.tanh}[cfg["activation"]]
    common = dict(data_id="tags", max_output_len=cfg["max_output_len"], hidden_dim=cfg["hidden_dim"], activation=act)
    if cfg["head"] == "sequence":
        dec = SequenceLabeler(name="tagger", encoders=encoders, vocabulary=tv, **common)
    else:
        dec = EmbeddingsLabeler(name="tagger", encoders=encoders, embedded_sequence=seq,
                                train_embeddings=cfg["train_embeddings"], **common)
    runner, xent = LabelRunner(output_series="tags", decoder=dec), XentRunner(output_series="xent", decoder=dec)
    trainer = CrossEntropyTrainer(decoders=[dec], l2_weight=0.0, clip_norm=None)
    tfm = TensorFlowManager(num_sessions=1, num_threads=1, device=str(dev), seed=1)
    tfm.initialize_sessions()
    return dict(seq=seq, encoders=encoders, dec=dec, runner=runner, xent=xent, trainer=trainer, tfm=tfm,
                feedables=feedables + [dec], store=tfm.sessions[0].store)


def dataset_of(z):
    """The fixture's strings: the source sentences, and one tag string per source word (an EmbeddingsLabeler's tags
    hold <pad> inside the sentence, which the vocabulary maps to 0 as the reference's did)."""
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    src = unpad(z["in/src_tokens"])
    tags = [[str(t) for t in row[:len(s)]] for row, s in zip(z["in/tgt_tokens"], src)]
    return Dataset("fixture", {"source": src, "tags": tags}, BatchingScheme(batch_size=len(src)))


def loaded(dev, case):
    z, cfg, params = load(case)
    m = build(dev, cfg)
    assert load_variables(m["store"], params) == []              # the same variables under the same names, both ways
    ds = dataset_of(z)
    fd = {}
    for part in m["feedables"]:
        fd.update(part.feed_dict(ds, train=False))
    assert np.array_equal(fd[m["dec"].train_tokens], z["in/tgt_ids"])
    return z, cfg, params, m, ds, fd


@pytest.mark.parametrize("case", FORWARD_CASES)
def test_engine_equals_the_reference(dev, case):
    z, cfg, _, m, ds, fd = loaded(dev, case)
    dec = m["dec"]
    fetches = {"logits": dec.logits, "logprobs": dec.logprobs, "train_xents": dec.train_xents, "cost": dec.cost,
               "decoded": dec.decoded, "labels": dec.labels, "input_mask": dec.input_mask}
    for i, enc in enumerate(m["encoders"]):
        fetches["enc{}_states".format(i)] = enc.temporal_states
    out = m["tfm"].sessions[0].run(fetches, fd)
    for key in ["enc{}_states".format(i) for i in range(len(m["encoders"]))] + ["logits", "logprobs", "train_xents",
                                                                                "cost"]:
        close(out[key], z["out/" + key], case + " " + key)
    assert np.array_equal(out["decoded"], z["out/decoded"])
    assert np.array_equal(out["input_mask"], z["out/input_mask"])
    assert np.array_equal(out["labels"], np.where(z["out/input_mask"] != 0, z["out/decoded"], R.END))
    assert not np.asarray(out["train_xents"])[z["in/tgt_ids"] == 0].any()               # exact zeros at <pad> targets
    res = m["tfm"].execute(ds, set(m["feedables"]), [m["runner"], m["xent"]], train=False, compute_losses=True)
    assert [" ".join(s) for s in res[0].outputs["tags"]] == [str(s) for s in z["out/runner_sentences"]]
    close(res[0].losses["tags/loss"], z["out/runner_loss"], case + " runner loss")
    close(np.asarray(res[1].outputs["xent"], np.float32), z["out/train_xents"], case + " XentRunner")
    # without targets: the same labels, no loss
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    bare = Dataset("bare", {"source": list(ds.get_series("source"))}, BatchingScheme(batch_size=len(ds)))
    res = m["tfm"].execute(bare, set(m["feedables"]), [m["runner"]], train=False, compute_losses=False)[0]
    assert [" ".join(s) for s in res.outputs["tags"]] == [str(s) for s in z["out/runner_sentences"]]


@pytest.mark.parametrize("case", ["fd_gradients_labeler", "fd_gradients_embeddings_labeler"])
def test_engine_gradients_against_the_reference_finite_differences(dev, case):
    z, _, _, m, ds, _ = loaded(dev, case)
    res = m["tfm"].execute(ds, m["trainer"].feedables, [m["trainer"]], train=True)[0]
    close(res.losses["tagger - cost"], z["out/cost"], "cost", 1e-4)
    store = m["store"]
    seen = set()
    for name, i, fd in zip([str(n) for n in z["fd/names"]], z["fd/index"], z["fd/value"]):
        got = float(store.g(name).reshape(-1)[int(i)])
        assert abs(got - fd) <= 6e-3 + 2e-2 * abs(fd), "{}[{}]: engine {:.6f} vs finite difference {:.6f}".format(
            name, i, got, fd)
        seen.add(name)
    assert seen == set(store.names())


def test_frozen_embeddings_cut_the_heads_share_of_the_tables_gradient_only(dev):
    """train_embeddings=False (tf.stop_gradient on the table in the head): the table still learns through the
    encoder's input, every other gradient is what it is with the share -- the two fixtures hold the same model."""
    grads = {}
    for case in ("embeddings_labeler_frozen", "embeddings_labeler_projected"):
        z, cfg, params = load(case)
        frozen, _, _ = load("embeddings_labeler_frozen")
        m = build(dev, cfg)
        load_variables(m["store"], {k[2:]: frozen[k] for k in frozen.files if k.startswith("p/")})
        m["tfm"].execute(dataset_of(frozen), m["trainer"].feedables, [m["trainer"]], train=True)
        grads[case] = {n: m["store"].g(n).detach().cpu().numpy().copy() for n in m["store"].names()}
    table = "encoder_input/embedding_matrix_0"
    a, b = grads["embeddings_labeler_frozen"], grads["embeddings_labeler_projected"]
    for name in a:
        if name != table:
            assert np.abs(a[name] - b[name]).max() <= 1e-6 * max(np.abs(b[name]).max(), 1e-3), name
    z, cfg, params = load("embeddings_labeler_frozen")
    states = [z["out/enc0_states"]]
    share = R.head(params, states, z["in/tgt_ids"], kind="embeddings", table=params[table])["grads"]["table"]
    assert np.abs(share).max() > 1e-3
    assert np.abs((b[table] - a[table]) - share).max() <= 1e-4 * np.abs(share).max()
    assert np.abs(a[table]).max() > 0                              # the encoder's scatter-add is still there


@pytest.mark.parametrize("case", ["fd_gradients_labeler", "embeddings_labeler_projected", "labeler_two_encoders"])
def test_head_gradients_against_float64_autograd(dev, case):
    """The head alone, the engine's own encoder states as the leaf."""
    from neuralmonkey_amd import ops
    from neuralmonkey_amd.runtime import RunContext
    z, cfg, params, m, ds, _ = loaded(dev, case)
    dec, sess, store = m["dec"], m["tfm"].sessions[0], m["store"]
    fd = {}
    for part in m["trainer"].feedables:
        fd.update(part.feed_dict(ds, train=True))
    ctx = RunContext(sess, fd)
    ops.zero(store.ensure_grad())
    sess.step_tensor()
    for part in m["trainer"].feedables:
        part.stage_inputs(ctx)
    count = dec.train_token_count(ctx)
    res = dec._train_loop(ctx, want_grad=True, grad_scale=torch.tensor([1.0 / count], device=dev))   # pylint: disable=protected-access
    states = [leaf.data.view(*shape).cpu().numpy().copy() for leaf, shape in zip(res.saved["leaves"], res.saved["shapes"])]
    res.saved["tape"].backward()
    torch.cuda.synchronize()
    d_states = np.concatenate([leaf.grad.view(*shape).cpu().numpy() for leaf, shape in
                               zip(res.saved["leaves"], res.saved["shapes"])], axis=2)
    cost = float(res.loss_sum.cpu()[0]) / count
    table = "encoder_input/embedding_matrix_0"
    head_vars = [n for n in store.names() if n.startswith("tagger/")]

    # float64 autograd
    tgt = torch.tensor(z["in/tgt_ids"].reshape(-1), dtype=torch.long)
    leaf = torch.tensor(np.concatenate(states, axis=2), dtype=torch.float64, requires_grad=True)
    p = {n: torch.tensor(params[n], dtype=torch.float64, requires_grad=True) for n in head_vars + [table]}
    h = leaf.reshape(-1, leaf.shape[2])
    if "tagger/hidden_layer/kernel" in p:
        h = {"relu": torch.relu, "tanh": torch.tanh}[cfg["activation"]](h @ p["tagger/hidden_layer/kernel"]
                                                                        + p["tagger/hidden_layer/bias"])
    if cfg["head"] == "sequence":
        logits = h @ p["tagger/logits/kernel"] + p["tagger/logits/bias"]
    else:
        if "tagger/project_for_embeddings/kernel" in p:
            h = h @ p["tagger/project_for_embeddings/kernel"] + p["tagger/project_for_embeddings/bias"]
        logits = h @ p[table].t()
    xent = torch.nn.functional.cross_entropy(logits, tgt, ignore_index=0, reduction="sum") / (float((tgt != 0).sum()) + 1e-9)
    xent.backward()
    xent = xent.detach()
    want = {n: p[n].grad.numpy() for n in head_vars}
    want["states"] = leaf.grad.numpy()
    if cfg["head"] == "embeddings":
        want["table"] = p[table].grad.numpy()

    kw = dict(kind=cfg["head"], activation=cfg["activation"], table=params[table])
    r64 = R.head(params, states, z["in/tgt_ids"], dtype=np.float64, **kw)
    r32 = R.head(params, states, z["in/tgt_ids"], dtype=np.float32, **kw)
    got = {n: store.g(n).detach().cpu().numpy() for n in head_vars}
    got["states"] = d_states
    if cfg["head"] == "embeddings":
        got["table"] = store.g(table).detach().cpu().numpy()      # (no encoder backward ran: the head's share alone)
    unit = max(abs(float(r32["cost"]) - float(r64["cost"])), EPS32 * abs(float(xent)))
    bound = min(MULTIPLE * unit, 1e-4 * abs(float(xent)))
    print("{} cost {:.6f}: error {:.3g} (unit {:.3g}, bound {:.3g})".format(case, cost, abs(cost - float(xent)), unit, bound))
    assert abs(float(r64["cost"]) - float(xent)) <= 1e-12 and abs(cost - float(xent)) <= bound
    for name in sorted(want):
        g64 = want[name]
        assert np.abs(r64["grads"][name] - g64).max() <= 1e-12, name        # the restatement's analytic gradient
        mag = float(np.abs(g64).max())
        unit = max(float(np.abs(r32["grads"][name] - g64).max()), EPS32 * mag)
        bound = min(MULTIPLE * unit, 1e-3 * mag)
        err = float(np.abs(got[name].astype(np.float64) - g64).max())
        print("{} d {}: error {:.3g} (unit {:.3g}, bound {:.3g}, magnitude {:.3g})".format(case, name, err, unit, bound,
                                                                                      mag))
        assert mag > 0 and err <= bound, (name, err, bound)


def _scheme(batch_size):
    from neuralmonkey_amd.dataset import BatchingScheme
    return BatchingScheme(batch_size=batch_size)


@pytest.mark.parametrize("name", ["labeler", "bert"])
def test_reference_ini_trains_and_labels(dev, ref_root, name):          # noqa: F811
    """30 training steps (DelayedUpdateTrainer: six updates) lower the cost of a held-out batch, evaluated without
    dropout before and after; LabelRunner returns one label per input token; XentRunner returns [B, T] xents that are
    zero where the target is <pad>."""
    from neuralmonkey_amd.runners import LabelRunner, XentRunner
    from .test_reference_inis import load_verbatim
    # (the files name their own tf_manager, which takes no seed from the loader: it is set the way the reference's
    # command line overrides a setting, so the run is the same every time -- dropout masks are functions of the step)
    model = load_verbatim(ref_root, name, device=str(dev), changes=["tf_manager.seed=1234"])
    assert model.tf_manager.seed == 1234
    tfm = model.tf_manager
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    label_runner = [r for r in model.runners if isinstance(r, LabelRunner)][0]
    dec = label_runner.decoder
    val = next(model.val_dataset.batches(_scheme(10)))
    assert len(val) == 10
    first = tfm.execute(val, feedables, [label_runner], compute_losses=True)[0].losses[label_runner.output_series + "/loss"]
    train_losses, steps = [], 0
    while steps < 30:
        for batch in model.train_dataset.batches(_scheme(10)):
            res = tfm.execute(batch, feedables, model.trainers, train=True)[0]
            train_losses.append(float(sum(v for k, v in res.losses.items() if k.endswith("cost"))))
            steps += 1
            if steps == 30:
                break
    assert tfm.sessions[0].global_step == 6 and np.isfinite(train_losses).all()
    out = tfm.execute(val, feedables, model.runners, compute_losses=True)
    last = out[model.runners.index(label_runner)].losses[label_runner.output_series + "/loss"]
    print("{}: held-out cost {:.4f} -> {:.4f}; training cost {:.4f} -> {:.4f}".format(name, first, last, train_losses[0],
                                                                                    train_losses[-1]))
    assert last < first
    sentences = out[model.runners.index(label_runner)].outputs[label_runner.output_series]
    # one label per input token: a sentence ends early only where the model itself predicts </s> (label_runner.py:34-43)
    fd = {}
    for part in feedables:
        fd.update(part.feed_dict(val, train=False))
    seen = tfm.sessions[0].run({"decoded": dec.decoded, "mask": dec.input_mask}, fd)
    lengths = np.asarray(seen["mask"]).sum(1).astype(int)
    source = list(val.get_series(dec.encoders[0].input_sequence.data_id))
    limit = dec.encoders[0].input_sequence.max_length or 10 ** 9
    assert lengths.tolist() == [min(len(s), limit) for s in source]
    assert sentences == R.runner_sentences(seen["decoded"], seen["mask"], dec.vocabulary.index_to_word)
    whole = [i for i, n in enumerate(lengths) if R.END not in np.asarray(seen["decoded"])[i, :n]]
    assert len(whole) >= 5 and all(len(sentences[i]) == lengths[i] for i in whole)
    if name == "bert":
        xent = [r for r in model.runners if isinstance(r, XentRunner)][0]
        table = np.asarray(out[model.runners.index(xent)].outputs["xent"])
        ids = dec.feed_dict(val, train=False)[dec.train_tokens]
        assert table.shape == ids.shape and not table[ids == 0].any() and (table[ids != 0] > 0).all()


def test_xent_runner_on_a_tagger(dev, tmp_path):
    model, (src, _) = M.load(tmp_path, "tagger", dev, runners="<runner>, <runner_xent>")
    batch = next(iter(model.train_dataset.batches()))
    feedables = set.union(*[r.feedables for r in model.runners])
    out = model.tf_manager.execute(batch, feedables, model.runners, compute_losses=True)
    table = np.asarray(out[1].outputs["xent"])
    ids = model.runners[0].decoder.feed_dict(batch, train=False)[model.runners[0].decoder.train_tokens]
    assert table.shape == ids.shape and not table[ids == 0].any() and (table[ids != 0] > 0).all()
    # one label per word, unless the (untrained) model itself predicts </s> inside the sentence
    dec = model.runners[0].decoder
    fd = {}
    for part in feedables:
        fd.update(part.feed_dict(batch, train=False))
    seen = model.tf_manager.sessions[0].run({"decoded": dec.decoded, "mask": dec.input_mask}, fd)
    assert np.asarray(seen["mask"]).sum(1).astype(int).tolist() == [len(s) for s in src]
    assert out[0].outputs["tags"] == R.runner_sentences(seen["decoded"], seen["mask"], dec.vocabulary.index_to_word)


def _mlm_batches(root):
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    out = []
    for seed, n in ((11, 6), (12, 4), (13, 6), (14, 4), (15, 6), (16, 4), (17, 6)):   # two shapes, three visits each
        rng = np.random.default_rng(seed)
        width = 7 if n == 6 else 5
        src = [[str(w) for w in rng.choice(M.WORDS, size=width if i == 0 else int(rng.integers(1, width + 1)))]
               for i in range(n)]
        tags = [[w if rng.random() < 0.6 or j == 0 else "<pad>" for j, w in enumerate(s)] for s in src]
        out.append(Dataset("b{}".format(seed), {"source": src, "tags": tags}, BatchingScheme(batch_size=n)))
    return out


def _train_mlm(dev, root, graphs):
    model, _ = M.load(root, "mlm", dev, keep=0.8)
    sess = model.tf_manager.sessions[0]
    sess.use_step_graphs = graphs
    trainer = model.trainers[0]
    losses = []
    for ds in _mlm_batches(root):
        res = model.tf_manager.execute(ds, trainer.feedables, [trainer], train=True)[0]
        losses.append(res.losses["tagger - cost"])
    replayed = sum(1 for st in sess.__dict__.get("_step_graphs", {}).values() if st[0] == 2)
    return np.asarray(losses), sess.store.state_dict(), replayed


def test_replayed_training_step_equals_eager(dev, tmp_path):
    """TransformerEncoder + EmbeddingsLabeler with dropout, the protocol of tests/test_step_graphs_gpu.py."""
    (tmp_path / "eager").mkdir()
    (tmp_path / "graph").mkdir()
    l_eager, p_eager, n_eager = _train_mlm(dev, tmp_path / "eager", False)
    l_graph, p_graph, n_graph = _train_mlm(dev, tmp_path / "graph", True)
    assert n_eager == 0
    assert n_graph >= 1, "no training step was captured: graph_safe_training refused this model"
    assert np.all(np.isfinite(l_graph))
    assert np.abs(l_graph - l_eager).max() <= 1e-5 * np.abs(l_eager).max(), (l_eager, l_graph)
    for name, want in p_eager.items():
        if name.endswith("keys_proj/bias"):
            continue        # its gradient is identically zero: Adam turns rounding noise into +-lr steps
        got = p_graph[name]
        assert np.abs(got - want).max() <= 1e-5 * max(float(np.abs(want).max()), 1e-3), name
    assert np.unique(np.round(l_graph, 6)).size > 3


@pytest.mark.parametrize("kind", ["tagger", "mlm"])
def test_a_labeler_step_launches_no_torch_kernels(dev, tmp_path, kind):
    from .test_no_foreign_kernels_gpu import _foreign_kernels
    model, _ = M.load(tmp_path, kind, dev, keep=0.9)
    ds = next(iter(model.train_dataset.batches()))
    trainer, runner = model.trainers[0], model.runners[0]
    foreign = _foreign_kernels(lambda: model.tf_manager.execute(ds, trainer.feedables, [trainer], train=True))
    assert not foreign, foreign
    foreign = _foreign_kernels(lambda: model.tf_manager.execute(ds, runner.feedables, [runner], compute_losses=True))
    assert not foreign, foreign
