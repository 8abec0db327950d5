"""Classifier / SequenceRegressor / the pooling encoders / the gradient-reversal views / LogitsRunner and
RegressionRunner on the MI355X.

  * every fixture of tests/golden/classifier (numbers of the REFERENCE'S OWN Python, see make_classifier_golden.py):
    the fixture's variables loaded by name, its strings fed; every fetched tensor within 1e-4 of the tensor's largest
    magnitude (``close`` of tests/test_reference_exec_gpu.py), decoded classes and GreedyRunner's words equal,
    LogitsRunner's strings parsed back to floats, RegressionRunner's predictions;
  * the engine's gradient against central differences of the reference's cost (6e-3 + 2e-2 |fd|);
  * the topology of the reference's tests/classifier.ini over fed states (relu, two decoders, one through a
    StatefulView) against torch autograd in float64: cost, every variable's gradient and d states by the unit method
    (unit = float32 evaluation of tests/pool_ref.py against float64, 16 units, capped by smoke()'s 1e-4 relative on the
    cost and 1e-3 of the largest magnitude on a gradient); each part's backward pass runs exactly once;
  * a classifier over a view and over the plain pooler: the head's gradients bit-equal, the encoder's exact negatives;
  * a captured and replayed training step over a Transformer encoder equals the eager one; no step launches a kernel
    of the tensor library; both of the reference's configurations train a few steps and decode."""
import numpy as np
import pytest
import torch

from . import classifier_models as M
from . import pool_ref as R
from .test_pool_host import ref_root, without_cnn_encoder  # noqa: F401  pylint: disable=unused-import
from .test_reference_exec_gpu import close

pytestmark = pytest.mark.gpu

MULTIPLE = 16.0
EPS32 = float(np.finfo(np.float32).eps)


def run_runner(m, runner, fd, sessions=1):
    ex = runner.get_executable(compute_losses=True, summaries=False, num_sessions=sessions)
    fetches, _ = ex.next_to_execute()
    ex.collect_results([m["tfm"].sessions[0].run(fetches, fd) for _ in range(sessions)])
    return ex.result


@pytest.mark.parametrize("case", M.FORWARD_CASES)
def test_engine_equals_the_reference(dev, case):
    z, cfg, _, m, ds, fd = M.loaded(dev, case)
    sess = m["tfm"].sessions[0]
    fetches = {"enc_states": m["enc"].temporal_states, "enc_mask": m["enc"].temporal_mask}
    for kind, part in m["readers"].items():
        fetches[kind + "_output"] = part.output
        if kind == "att":
            fetches.update(att_weights=part.attention_weights, att_temporal_states=part.temporal_states,
                           att_temporal_mask=part.temporal_mask)
    dec = m["dec"]
    if cfg["head"] == "classifier":
        assert np.array_equal(fd[dec.targets_placeholder], z["in/tgt_ids"])
        fetches.update(decoded_seq=dec.decoded_seq, decoded_logits=dec.decoded_logits,
                       runtime_logprobs=dec.runtime_logprobs, cost=dec.cost)
    elif cfg["head"] == "regressor":
        assert np.array_equal(fd[dec.targets_placeholder], z["in/targets"])
        fetches.update(predictions=dec.predictions, cost=dec.cost)
    out = sess.run(fetches, fd)
    for key in fetches:
        if key in ("decoded_seq", "enc_mask", "att_temporal_mask"):
            assert np.array_equal(out[key], z["out/" + key]), key
        else:
            close(out[key], z["out/" + key], case + " " + key)
    if cfg["head"] == "classifier":
        for sessions in (1, 2):                                   # one session: argmax on the device; several: logaddexp
            res = run_runner(m, m["runners"]["greedy"], fd, sessions)
            assert [" ".join(s) for s in res.outputs["cls"]] == [str(s) for s in z["out/runner_greedy"]]
            close(np.asarray(sorted(res.losses.values())) / sessions, np.sort(z["out/runner_greedy_losses"]),
                  case + " greedy losses")
        for tag in ("logits", "logits_raw_pick0", "logits_pick"):
            res = run_runner(m, m["runners"][tag], fd)
            mine = R.parse_logits_strings(res.outputs["dist"])
            theirs = R.parse_logits_strings([[str(s)] for s in z["out/runner_" + tag]])
            close(mine, theirs, case + " runner " + tag)
        res = m["tfm"].execute(ds, set(m["feedables"]), [m["runners"]["greedy"], m["runners"]["logits"]], train=False,
                               compute_losses=True)
        assert [" ".join(s) for s in res[0].outputs["cls"]] == [str(s) for s in z["out/runner_greedy"]]
        # without targets: the same classes, no loss
        from neuralmonkey_amd.dataset import BatchingScheme, Dataset
        bare = Dataset("bare", {"source": list(ds.get_series("source"))}, BatchingScheme(batch_size=len(ds)))
        res = m["tfm"].execute(bare, set(m["feedables"]), [m["runners"]["greedy"]], train=False, compute_losses=False)
        assert [" ".join(s) for s in res[0].outputs["cls"]] == [str(s) for s in z["out/runner_greedy"]]
    elif cfg["head"] == "regressor":
        res = run_runner(m, m["runners"]["regression"], fd)
        close(np.asarray(res.outputs["reg"], np.float32), z["out/runner_predictions"], case + " runner predictions")
        close(res.losses["reg/mse"], z["out/runner_mse"], case + " runner mse")


@pytest.mark.parametrize("case", M.FD_CASES)
def test_engine_gradients_against_the_reference_finite_differences(dev, case):
    z, cfg, _, m, ds, _ = M.loaded(dev, case)
    res = m["tfm"].execute(ds, m["trainer"].feedables, [m["trainer"]], train=True)[0]
    close(res.losses["{} - cost".format(cfg["head"])], z["out/cost"], "cost", 1e-4)
    store = m["store"]
    seen = set()
    for name, i, fd in zip([str(n) for n in z["fd/names"]], z["fd/index"], z["fd/value"]):
        got = float(store.g(name).reshape(-1)[int(i)])
        print("{}[{}]: engine {:.6f} finite difference {:.6f}".format(name, i, got, fd))
        assert abs(got - fd) <= 6e-3 + 2e-2 * abs(fd), "{}[{}]: engine {:.6f} vs finite difference {:.6f}".format(
            name, i, got, fd)
        seen.add(name)
    assert seen == set(store.names())


def count_calls(parts):
    """Wrap ``backward`` of every part; -> the list the calls are logged to."""
    log = []
    for name, part in parts.items():
        inner = part.backward

        def wrapped(ctx, d_states, d_final=None, _inner=inner, _name=name, _part=part):
            log.append(_name)
            if d_states is not None:
                _part.last_d_states = d_states.detach().clone()
            return _inner(ctx, d_states, d_final)
        part.backward = wrapped
    return log


def test_adversarial_topology_against_float64_autograd(dev):
    from .test_pool_host import _t, torch_attentive, torch_classifier_cost, torch_max_pool
    m = M.build_topology(dev)
    ds = M.topology_dataset()
    log = count_calls({"att": m["att"], "pool": m["pool"], "view": m["view"], "filler": m["filler"]})
    store = m["store"]
    params = {n: store[n].detach().cpu().numpy().astype(np.float64) for n in store.names()}
    res = m["tfm"].execute(ds, m["trainer"].feedables, [m["trainer"]], train=True)[0]
    torch.cuda.synchronize()
    assert sorted(log) == ["att", "filler", "pool", "view"], log           # each part's backward exactly once
    assert log.index("view") < log.index("pool") < log.index("filler") and log.index("att") < log.index("filler")
    cost = float(res.losses["classifier - cost"]) + float(res.losses["classifier_adv - cost"])

    class Reverse(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.view_as(x)

        @staticmethod
        def backward(ctx, grad):
            return -grad
    fd = m["filler"].feed_dict(ds, train=True)
    x = np.asarray(fd[m["filler"].states_input], np.float64)
    lengths = np.asarray(fd[m["filler"].lengths_input])
    mask = (np.arange(x.shape[1])[None, :] < lengths[:, None]).astype(np.float64)
    ids = np.asarray(m["main"].feed_dict(ds, train=True)[m["main"].targets_placeholder])
    p = {n: _t(v) for n, v in params.items()}
    xt, mt = _t(x), _t(mask, False)
    pooled = torch_max_pool(xt, mt)
    main = torch_classifier_cost(p, torch.cat([torch_attentive(p, xt, mt, "encoder_att"), pooled], dim=1), ids,
                                 "classifier", 1, "relu")
    adv = torch_classifier_cost(p, Reverse.apply(pooled), ids, "classifier_adv", 0, "relu")
    (main + adv).backward()
    want = {n: p[n].grad.numpy() for n in params}
    want["states"] = xt.grad.numpy()
    r64 = R.adversarial_topology(params, x, mask, ids, 1, "relu", np.float64)
    r32 = R.adversarial_topology(params, x, mask, ids, 1, "relu", np.float32)
    total = float((main + adv).detach())
    unit = max(abs(float(r32["cost"]) - total), EPS32 * abs(total))
    bound = min(MULTIPLE * unit, 1e-4 * abs(total))
    print("cost {:.6f}: error {:.3g} (unit {:.3g}, bound {:.3g})".format(cost, abs(cost - total), unit, bound))
    assert abs(float(r64["cost"]) - total) <= 1e-12 and abs(cost - total) <= bound
    got = {n: store.g(n).detach().cpu().numpy() for n in params}
    got["states"] = m["filler"].last_d_states.cpu().numpy()
    for name in sorted(want):
        g64 = want[name]
        assert np.abs(r64["grads"][name] - g64).max() <= 1e-12, name
        mag = float(np.abs(g64).max())
        unit = max(float(np.abs(r32["grads"][name].astype(np.float64) - g64).max()), EPS32 * mag)
        bound = min(MULTIPLE * unit, 1e-3 * mag)
        err = float(np.abs(got[name].astype(np.float64) - g64).max())
        print("d {}: error {:.3g} (unit {:.3g}, bound {:.3g}, magnitude {:.3g})".format(name, err, unit, bound, mag))
        assert mag > 0 and err <= bound, (name, err, bound)
    # the tie of sentence 0: both positions took a share of the pooler's gradient
    assert got["states"][0, 1, 0] != 0 and got["states"][0, 4, 0] != 0


def test_a_view_negates_the_encoders_gradient_exactly(dev):
    """The same classifier over a StatefulView of the pooler and over the pooler itself: equal cost, bit-equal head
    gradients, exactly negated gradients of EVERY variable behind the view.  No word of the batch occurs more than
    twice: the embedding scatter-add (nm_embedding_scatter_add) sums the rows of a repeated word with float atomics in
    an order that varies from run to run, and only a sum of two terms is independent of its order."""
    from collections import Counter
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    z, cfg, params = M.load_fixture("classifier_no_layers")
    words = ["w{}".format(i % cfg["src_vocab"]) for i in range(21)]           # w0 .. w16, then w0 .. w3 again
    words[5] = words[9] = "never-seen"                                          # <unk> twice, too
    source, at = [], 0
    for n in (4, 7, 3, 6, 1):
        source.append(words[at:at + n])
        at += n
    assert max(Counter(w for s in source for w in s).values()) == 2
    ds = Dataset("twice", {"source": source, "target": [[str(t)] for t in z["in/tgt_tokens"]]},
                 BatchingScheme(batch_size=len(source)))
    grads, costs = {}, {}
    for through in (False, True):
        m = M.build(dev, dict(cfg, encoders=["max"], through_views=through))
        m["store"].load_state_dict({n: v for n, v in params.items() if n in set(m["store"].names())}, strict=False)
        res = m["tfm"].execute(ds, m["trainer"].feedables, [m["trainer"]], train=True)[0]
        costs[through] = float(res.losses["classifier - cost"])
        grads[through] = {n: m["store"].g(n).detach().cpu().numpy().copy() for n in m["store"].names()}
    assert costs[False] == costs[True]
    plain, viewed = grads[False], grads[True]
    head = [n for n in plain if n.startswith("classifier/")]
    behind = [n for n in plain if not n.startswith("classifier/")]
    assert len(head) == 2 and len(behind) >= 9 and "encoder_input/embedding_matrix_0" in behind
    for n in head:
        assert np.array_equal(plain[n], viewed[n]) and np.abs(plain[n]).max() > 0, n
    for n in behind:
        assert np.array_equal(viewed[n], -plain[n]), n
    assert sum(float(np.abs(plain[n]).max()) > 0 for n in behind) >= 8


def _batches():
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    out = []
    for seed, n in ((11, 6), (12, 4), (13, 6), (14, 4), (15, 6), (16, 4), (17, 6)):   # two shapes, three visits each
        rng = np.random.default_rng(seed)
        width = 7 if n == 6 else 5
        src = [[str(w) for w in rng.choice(M.WORDS, size=width if i == 0 else int(rng.integers(1, width + 1)))]
               for i in range(n)]
        cls = [[M.CLASSES[int(s[0][1:]) % len(M.CLASSES)]] for s in src]
        count = [np.asarray([len(s)], np.float32) for s in src]
        out.append(Dataset("b{}".format(seed), {"source": src, "cls": cls, "count": count},
                           BatchingScheme(batch_size=n)))
    return out


def _train(dev, root, graphs):
    model, _ = M.load_ini(root, dev, keep=0.8)
    sess = model.tf_manager.sessions[0]
    sess.use_step_graphs = graphs
    trainer = model.trainers[0]
    losses = []
    for ds in _batches():
        res = model.tf_manager.execute(ds, trainer.feedables, [trainer], train=True)[0]
        losses.append([res.losses[k] for k in ("decoder - cost", "decoder_adv - cost", "regressor - cost")])
    replayed = sum(1 for st in sess.__dict__.get("_step_graphs", {}).values() if st[0] == 2)
    return np.asarray(losses), sess.store.state_dict(), replayed


def test_replayed_training_step_equals_eager(dev, tmp_path):
    """TransformerEncoder under AttentiveEncoder + both poolers, two Classifiers (one through a view) and a
    SequenceRegressor, with dropout: the protocol of tests/test_step_graphs_gpu.py."""
    (tmp_path / "eager").mkdir()
    (tmp_path / "graph").mkdir()
    l_eager, p_eager, n_eager = _train(dev, tmp_path / "eager", False)
    l_graph, p_graph, n_graph = _train(dev, tmp_path / "graph", True)
    assert n_eager == 0
    assert n_graph >= 1, "no training step was captured: graph_safe_training refused this model"
    assert np.all(np.isfinite(l_graph))
    assert np.abs(l_graph - l_eager).max() <= 1e-5 * np.abs(l_eager).max(), (l_eager, l_graph)
    for name, want in p_eager.items():
        if name.endswith("keys_proj/bias"):
            continue        # its gradient is identically zero: Adam turns rounding noise into +-lr steps
        got = p_graph[name]
        assert np.abs(got - want).max() <= 1e-5 * max(float(np.abs(want).max()), 1e-3), name
    assert np.unique(np.round(l_graph[:, 0], 6)).size > 3


def test_a_step_launches_no_torch_kernels(dev, tmp_path):
    from .test_no_foreign_kernels_gpu import _foreign_kernels
    model, _ = M.load_ini(tmp_path, dev, keep=0.9)
    ds = next(iter(model.train_dataset.batches()))
    trainer = model.trainers[0]
    foreign = _foreign_kernels(lambda: model.tf_manager.execute(ds, trainer.feedables, [trainer], train=True))
    assert not foreign, foreign
    feedables = set.union(*[r.feedables for r in model.runners])
    foreign = _foreign_kernels(lambda: model.tf_manager.execute(ds, feedables, model.runners, compute_losses=True))
    assert not foreign, foreign


def test_sentence_heads_learn_and_decode(dev, tmp_path):
    """The class is a function of the first word, the regression target the sentence length: 60 steps lower both costs;
    the runners return one class / one distribution / one prediction per sentence."""
    model, src = M.load_ini(tmp_path, dev)
    tfm, trainer = model.tf_manager, model.trainers[0]
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    ds = next(iter(model.train_dataset.batches()))
    losses = []
    for _ in range(60):
        res = tfm.execute(ds, feedables, [trainer], train=True)[0]
        losses.append([float(res.losses["decoder - cost"]), float(res.losses["regressor - cost"])])
    losses = np.asarray(losses)
    print("classifier cost {:.4f} -> {:.4f}; regressor cost {:.4f} -> {:.4f}".format(
        losses[0, 0], losses[-1, 0], losses[0, 1], losses[-1, 1]))
    assert np.isfinite(losses).all() and (losses[-1] < losses[0]).all()
    greedy, logits, reg = tfm.execute(ds, feedables, model.runners, compute_losses=True)
    assert len(greedy.outputs["cls"]) == len(src) and all(len(s) <= 1 for s in greedy.outputs["cls"])
    dist = R.parse_logits_strings(logits.outputs["distribution"])
    assert dist.shape == (len(src), 4 + len(M.CLASSES)) and np.allclose(dist.sum(axis=1), 1.0, atol=1e-5)
    words = model.runners[0].decoder.vocabulary.index_to_word
    best = [words[i] for i in dist.argmax(axis=1)]
    assert [s[0] for s in greedy.outputs["cls"] if s] == [w for w, s in zip(best, greedy.outputs["cls"]) if s]
    pred = np.asarray(reg.outputs["count"])
    assert pred.shape == (len(src), 1) and np.isfinite(pred).all()
    assert abs(float(reg.losses["count/mse"]) - float(np.mean((pred[:, 0] - [len(s) for s in src]) ** 2))) <= 1e-3 * max(
        1.0, float(reg.losses["count/mse"]))


@pytest.mark.parametrize("name", ["classifier", "regressor"])
def test_reference_ini_trains_and_decodes(dev, ref_root, name):          # noqa: F811
    """tests/regressor.ini verbatim, tests/classifier.ini without its SequenceCNNEncoder: a few optimizer steps with
    dropout, then every runner of the file on a validation batch."""
    from neuralmonkey_amd.dataset import BatchingScheme
    from .test_reference_inis import load_verbatim
    ini = without_cnn_encoder(ref_root) if name == "classifier" else name
    model = load_verbatim(ref_root, ini, device=str(dev), changes=["tf_manager.seed=1234"])
    tfm = model.tf_manager
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    val = next(model.val_dataset.batches(BatchingScheme(batch_size=10)))
    costs, steps = [], 0
    for batch in model.train_dataset.batches(BatchingScheme(batch_size=16)):
        res = tfm.execute(batch, feedables, model.trainers, train=True)[0]
        costs.append(float(sum(v for k, v in res.losses.items() if k.endswith("cost"))))
        steps += 1
        if steps == 8:
            break
    assert steps == 8 and tfm.sessions[0].global_step == 8 and np.isfinite(costs).all()
    out = tfm.execute(val, feedables, model.runners, compute_losses=True)
    if name == "classifier":
        dec = model.runners[0].decoder
        words = out[0].outputs["classification"]
        assert len(words) == 10 and all(len(s) <= 1 for s in words)
        dist = R.parse_logits_strings(out[1].outputs["distribution"])
        assert dist.shape == (10, len(dec.vocabulary)) and np.allclose(dist.sum(axis=1), 1.0, atol=1e-5)
        best = [dec.vocabulary.index_to_word[i] for i in dist.argmax(axis=1)]
        assert [s[0] for s in words if s] == [w for w, s in zip(best, words) if s]      # the two runners agree
        assert np.isfinite(list(out[0].losses.values())).all() and np.isfinite(list(out[1].losses.values())).all()
    else:
        pred = np.asarray(out[0].outputs["regression"])
        assert pred.shape == (10, 1) and np.isfinite(pred).all()
        want = np.asarray([row[0] for row in val.get_series("regression")], np.float64)
        mse = float(out[0].losses["regression/mse"])
        assert abs(mse - float(np.mean((pred[:, 0] - want) ** 2))) <= 1e-4 * max(1.0, mse)
