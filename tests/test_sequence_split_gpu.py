"""SequenceSplitter, the gradient-blocking views and word2vec-initialised embeddings on the MI355X.

  * the split alone over fed states (B = 3, T = 5, lengths 5 / 3 / 1, D = 12, factors 1 .. 4): the states are NumPy's
    reshape bit for bit IN the parent's storage, mask and int32 lengths exact, the gradient back at the parent bit for
    bit and in the reader's storage;
  * with a projection (P in {24, 36}, B*T in {15, 33}, none / relu / tanh): pre-activations, dW, db and dx against a
    float64 NumPy restatement written out here, each element under (n + 2) * 2^-24 * (the sum of the absolute values of
    its n products [+ |b|]) -- the worst-case bound of an fp32 sum of n products in any order; with tanh the tolerance of
    tests/test_tape_gpu.py's tanh-epilogue test (``close`` of tests/tape_ref.py);
  * blocking views over a tiny SentenceEncoder under a Decoder, on the hand-scheduled and on the taped path: read only
    through views the encoder's variables, gradient slices and optimizer slots stay as they are (after a step of a
    direct reader in the same session, and under DelayedUpdateTrainer); read directly as well, its gradient is bit-equal
    to the model without the second head;
  * the non-autoregressive model from INI text (TransformerEncoder -> SequenceSplitter -> TransformerEncoder ->
    CTCDecoder) learns four sentences; tests/language-model.ini verbatim initialises from sample.w2v, trains and scores.
"""
import numpy as np
import pytest
import torch

from . import tape_ref as R
from .test_sequence_split_host import lm_root, sample_rows  # noqa: F401  pylint: disable=unused-import

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


# ---- the splitter over fed states ---------------------------------------------------------------------------------------
def _fed_model(dev, lengths, d, factor, projection_size=None, activation=None, seed=0, train=True):
    from neuralmonkey_amd import tf_shim
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    from neuralmonkey_amd.encoders.numpy_stateful_filler import TemporalFiller
    from neuralmonkey_amd.model.sequence_split import SequenceSplitter
    from neuralmonkey_amd.runtime import RunContext, reset_registry
    from neuralmonkey_amd.tf_manager import TensorFlowManager
    reset_registry()
    rng = np.random.default_rng(seed)
    filler = TemporalFiller(name="states", data_id="features", input_size=d)
    act = {None: None, "relu": tf_shim.nn.relu, "tanh": tf_shim.tanh}[activation]
    split = SequenceSplitter("splitter", filler, factor, projection_size=projection_size, projection_activation=act)
    tfm = TensorFlowManager(num_sessions=1, num_threads=1, device=str(dev), seed=1)
    tfm.initialize_sessions()
    sess = tfm.sessions[0]
    feats = [rng.standard_normal((n, d)).astype(np.float32) for n in lengths]
    ds = Dataset("fed", {"features": feats}, BatchingScheme(batch_size=len(feats)))
    fd = {}
    for part in (filler, split):
        fd.update(part.feed_dict(ds, train=train))
    ctx = RunContext(sess, fd)
    received = []
    filler.backward = lambda ctx, d_states, d_final=None: received.append((d_states, d_final))
    return filler, split, sess, ctx, fd, received, rng


@pytest.mark.parametrize("factor", [1, 2, 3, 4])
def test_split_alone_is_a_view_with_exact_mask_and_lengths(dev, factor):
    lengths, d = (5, 3, 1), 12
    filler, split, _, ctx, fd, received, rng = _fed_model(dev, lengths, d, factor)
    ctx.memo["want_backward"] = True
    bsz, steps = len(lengths), max(lengths)
    assert split.dimension == d // factor
    parent = filler.temporal_states(ctx)
    states = split.temporal_states(ctx)
    assert tuple(states.shape) == (bsz, steps * factor, d // factor) and states.is_contiguous()
    assert states.data_ptr() == parent.data_ptr()
    assert states.untyped_storage().data_ptr() == parent.untyped_storage().data_ptr()
    fed = fd[filler.states_input]
    assert fed.shape == (bsz, steps, d)
    assert np.array_equal(states.cpu().numpy(), fed.reshape(bsz, steps * factor, d // factor))
    mask, lens = split.temporal_mask(ctx), split.lengths(ctx)
    want_mask = (np.arange(steps)[None, :] < np.asarray(lengths)[:, None]).astype(np.float32)
    assert mask.dtype == torch.float32 and np.array_equal(mask.cpu().numpy(), np.repeat(want_mask, factor, axis=1))
    assert lens.dtype == torch.int32 and lens.cpu().numpy().tolist() == [n * factor for n in lengths]
    assert split.graph_safe_training(True) is True
    # backward: handed on through defer_backward, once, the reader's own memory viewed back
    grad = torch.from_numpy(rng.standard_normal((bsz, steps * factor, d // factor)).astype(np.float32)).to(dev)
    kept = grad.clone()
    ctx.memo["backward_deferred"] = True
    split.backward(ctx, grad)
    assert received == []
    ctx.flush_backward()
    (got, final), = received
    assert final is None and tuple(got.shape) == (bsz, steps, d) and got.data_ptr() == grad.data_ptr()
    assert torch.equal(got.reshape(-1), kept.reshape(-1))
    # two readers, one of which calls backward itself as the recurrent and Transformer encoders do: one pass, on the sum
    del received[:]
    other = torch.from_numpy(rng.standard_normal(tuple(grad.shape)).astype(np.float32)).to(dev)
    ctx.defer_backward(split, grad, None)
    split.backward(ctx, other)
    ctx.flush_backward()
    (got, _), = received
    assert torch.equal(got.reshape(-1), (kept + other).reshape(-1)) and torch.equal(grad, kept)


def _projection_reference(x, w, b, activation, dy, dtype):
    """(pre-activation, output, dW, db, dx) by torch autograd on the CPU in ``dtype``."""
    xt, wt, bt = (torch.tensor(v, dtype=dtype, requires_grad=True) for v in (x, w, b))
    pre = xt @ wt + bt
    out = {None: lambda v: v, "relu": torch.relu, "tanh": torch.tanh}[activation](pre)
    out.backward(torch.tensor(dy, dtype=dtype))
    return pre.detach(), out.detach(), wt.grad, bt.grad, xt.grad


@pytest.mark.parametrize("activation", [None, "relu", "tanh"])
@pytest.mark.parametrize("lengths", [(5, 3, 1), (11, 4, 1)])
@pytest.mark.parametrize("width", [24, 36])
def test_projection_against_float64(dev, width, lengths, activation):
    d, factor = 12, 4
    filler, split, sess, ctx, fd, received, rng = _fed_model(dev, lengths, d, factor, width, activation,
                                                             seed=width + len(lengths) + max(lengths))
    ctx.memo["want_backward"] = True
    bsz, steps = len(lengths), max(lengths)
    rows = bsz * steps
    assert rows in (15, 33)
    w = rng.uniform(-0.6, 0.6, (d, width)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, (width,)).astype(np.float32)
    store = sess.store
    store["splitter/dense/kernel"].copy_(torch.from_numpy(w))
    store["splitter/dense/bias"].copy_(torch.from_numpy(b))
    x = fd[filler.states_input].reshape(rows, d)
    dy = rng.standard_normal((rows, width)).astype(np.float32)
    # the float64 restatement
    x64, w64, b64, dy64 = (v.astype(np.float64) for v in (x, w, b, dy))
    pre64 = x64 @ w64 + b64
    pre_bound = (d + 2) * U * (np.abs(x64) @ np.abs(w64) + np.abs(b64))
    if activation == "relu":
        assert (np.abs(pre64)[x.any(axis=1)] > 4 * pre_bound[x.any(axis=1)]).all(), "a pre-activation too close to 0"
    out64 = {None: lambda v: v, "relu": lambda v: np.maximum(v, 0), "tanh": np.tanh}[activation](pre64)
    dpre64 = {None: dy64, "relu": dy64 * (pre64 > 0), "tanh": dy64 * (1 - out64 ** 2)}[activation]
    want = {"dW": x64.T @ dpre64, "db": dpre64.sum(0), "dx": dpre64 @ w64.T}
    bound = {"dW": (rows + 2) * U * (np.abs(x64).T @ np.abs(dpre64)), "db": (rows + 2) * U * np.abs(dpre64).sum(0),
             "dx": (width + 2) * U * (np.abs(dpre64) @ np.abs(w64).T)}
    # the engine
    states = split.temporal_states(ctx)
    assert tuple(states.shape) == (bsz, steps * factor, width // factor) and states.is_contiguous()
    act = split._activations(ctx)                                  # pylint: disable=protected-access
    assert states.data_ptr() == act["out"].data_ptr() and tuple(act["out"].shape) == (rows, width)
    out = states.cpu().numpy().reshape(rows, width).astype(np.float64)
    grad = torch.from_numpy(dy).to(dev).view(bsz, steps * factor, width // factor)
    ctx.memo["backward_deferred"] = True
    split.backward(ctx, grad)
    ctx.flush_backward()
    (dx, final), = received
    assert final is None and tuple(dx.shape) == (bsz, steps, d)
    got = {"dW": store.g("splitter/dense/kernel").cpu().numpy().astype(np.float64),
           "db": store.g("splitter/dense/bias").cpu().numpy().astype(np.float64),
           "dx": dx.cpu().numpy().reshape(rows, d).astype(np.float64)}
    assert torch.equal(grad.cpu().reshape(-1), torch.from_numpy(dy).reshape(-1)), "the reader's gradient was overwritten"
    if activation == "tanh":
        ref64 = _projection_reference(x, w, b, activation, dy, torch.float64)
        ref32 = _projection_reference(x, w, b, activation, dy, torch.float32)
        label = "splitter tanh {} x {}".format(rows, width)
        R.close(label, "value", torch.from_numpy(out), ref64[1], ref32[1])
        for name, i in (("dW", 2), ("db", 3), ("dx", 4)):
            R.close(label, "grad " + name, torch.from_numpy(got[name]), ref64[i], ref32[i])
        # ... and where nothing is recorded the tanh sits in the product's epilogue: the same tolerance
        _, split2, sess2, ctx2, _, _, _ = _fed_model(dev, lengths, d, factor, width, activation,
                                                     seed=width + len(lengths) + max(lengths), train=False)
        sess2.store["splitter/dense/kernel"].copy_(torch.from_numpy(w))
        sess2.store["splitter/dense/bias"].copy_(torch.from_numpy(b))
        plain = split2.temporal_states(ctx2)
        assert not split2._activations(ctx2)["tape"].recording      # pylint: disable=protected-access
        R.close(label, "value (epilogue)", plain.cpu().reshape(rows, width).double(), ref64[1], ref32[1])
        return
    err = np.abs(out - out64)
    print("{} rows x {} {}: value error / bound {:.3f}".format(rows, width, activation, (err / pre_bound).max()))
    assert (err <= pre_bound).all()
    for name in ("dW", "db", "dx"):
        err = np.abs(got[name] - want[name])
        ok = bound[name] > 0
        print("    {} error / bound {:.3f}".format(name, (err[ok] / bound[name][ok]).max() if ok.any() else 0.0))
        assert (err <= bound[name]).all(), name


def test_a_parent_that_hands_out_a_column_slice(dev):
    """States that are columns 4..15 of a 20-wide buffer: without a projection they cannot be regrouped in place and are
    packed by the library's strided copy (equal values, other storage); a projection reads them through their row stride."""
    from neuralmonkey_amd.model.model_part import ModelPart
    from neuralmonkey_amd.model.sequence_split import SequenceSplitter
    from neuralmonkey_amd.model.stateful import TemporalStateful
    from neuralmonkey_amd.runtime import RunContext, reset_registry, tensor

    class Sliced(ModelPart, TemporalStateful):
        dimension = 12

        @tensor
        def temporal_states(self, ctx):
            return self.wide[:, :, 4:16]

        @tensor
        def temporal_mask(self, ctx):
            return self.mask

        def backward(self, ctx, d_states, d_final=None):
            self.received = d_states
    reset_registry()
    rng = np.random.default_rng(9)
    parent = Sliced("sliced")
    plain = SequenceSplitter("plain", parent, 3)
    projected = SequenceSplitter("projected", parent, 2, projection_size=24)
    _, sess = _session(dev)
    wide = rng.standard_normal((3, 5, 20)).astype(np.float32)
    parent.wide = torch.from_numpy(wide).to(dev)
    parent.mask = torch.ones(3, 5, device=dev)
    fd = {}
    for part in (parent, plain, projected):
        fd.update(part.feed_dict([0, 1, 2], train=True))
    ctx = RunContext(sess, fd)
    got = plain.temporal_states(ctx)
    assert got.is_contiguous() and np.array_equal(got.cpu().numpy(), wide[:, :, 4:16].reshape(3, 15, 4))
    assert got.untyped_storage().data_ptr() != parent.wide.untyped_storage().data_ptr()
    grad = torch.from_numpy(rng.standard_normal((3, 15, 4)).astype(np.float32)).to(dev)
    plain.backward(ctx, grad)
    assert tuple(parent.received.shape) == (3, 5, 12) and torch.equal(parent.received.reshape(-1), grad.reshape(-1))
    w = rng.uniform(-0.6, 0.6, (12, 24)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, (24,)).astype(np.float32)
    sess.store["projected/dense/kernel"].copy_(torch.from_numpy(w))
    sess.store["projected/dense/bias"].copy_(torch.from_numpy(b))
    out = projected.temporal_states(ctx).cpu().numpy().reshape(15, 24).astype(np.float64)
    x64 = wide[:, :, 4:16].reshape(15, 12).astype(np.float64)
    want = x64 @ w.astype(np.float64) + b.astype(np.float64)
    bound = (12 + 2) * U * (np.abs(x64) @ np.abs(w.astype(np.float64)) + np.abs(b.astype(np.float64)))
    assert (np.abs(out - want) <= bound).all()


def test_every_kind_of_reader_over_one_splitter(dev):
    """A recurrent encoder, an attention, a pooling encoder and a CTC head all read ONE splitter (two objectives): the
    splitter's backward pass and its parent's each run once per step, on the sum of what the readers sent."""
    from neuralmonkey_amd import tf_shim
    from neuralmonkey_amd.attention import Attention
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    from neuralmonkey_amd.decoders import CTCDecoder, Decoder
    from neuralmonkey_amd.encoders import RecurrentEncoder, SequenceAveragePooling
    from neuralmonkey_amd.encoders.numpy_stateful_filler import TemporalFiller
    from neuralmonkey_amd.model.sequence_split import SequenceSplitter
    from neuralmonkey_amd.runtime import reset_registry
    from neuralmonkey_amd.trainers import CrossEntropyTrainer
    reset_registry()
    filler = TemporalFiller(name="states", data_id="features", input_size=12)
    split = SequenceSplitter("splitter", filler, 2, projection_size=16, projection_activation=tf_shim.tanh)
    rnn = RecurrentEncoder(name="rnn", input_sequence=split, rnn_layers=[(8, "bidirectional", "GRU")])
    pool = SequenceAveragePooling("pool", split)
    att = Attention(name="attention", encoder=split)
    dec = Decoder(encoders=[rnn, pool], vocabulary=_vocab(), data_id="target", name="decoder", max_output_len=6,
                  embedding_size=8, rnn_size=8, attentions=[att])
    ctc = CTCDecoder("ctc", split, _vocab(), "target")
    trainer = CrossEntropyTrainer(decoders=[dec, ctc], l2_weight=0.0, clip_norm=None)
    tfm, sess = _session(dev)
    calls = {"received": 0, "splitter": 0, "states": 0}
    receive, replay = split.backward, split._replay                 # pylint: disable=protected-access

    def received(ctx, d_states, d_final=None):
        calls["received"] += 1
        receive(ctx, d_states, d_final)

    def replayed(ctx, d_states):
        calls["splitter"] += 1
        assert tuple(d_states.shape)[1:] == (10, 8)
        replay(ctx, d_states)

    def parent(ctx, d_states, d_final=None):
        calls["states"] += 1
        assert tuple(d_states.shape)[1:] == (5, 12) and bool(torch.isfinite(d_states).all())
    split.backward, split._replay, filler.backward = received, replayed, parent      # pylint: disable=protected-access
    rng = np.random.default_rng(3)
    feats = [rng.standard_normal((n, 12)).astype(np.float32) for n in (5, 3, 2, 4)]
    ds = Dataset("fed", {"features": feats, "target": TARGET}, BatchingScheme(batch_size=4))
    assert split in trainer.feedables and filler in trainer.feedables
    for step in (1, 2):
        res = tfm.execute(ds, trainer.feedables, [trainer], train=True)[0]
        assert np.isfinite([float(res.losses["decoder - cost"]), float(res.losses["ctc - cost"])]).all()
        # the recurrent encoder calls its input's backward itself, the other three readers defer theirs (two decoders)
        assert calls == {"received": 2 * step, "splitter": step, "states": step}
        for n in ("splitter/dense/kernel", "splitter/dense/bias"):
            assert float(sess.store.g(n).abs().max()) > 0, n


# ---- blocking views ---------------------------------------------------------------------------------------------------------
WORDS = ["w{}".format(i) for i in range(12)]
# no word more than twice: the embedding scatter-add sums a repeated word's rows with float atomics, and only a sum of two
# terms is independent of its order
SOURCE = [WORDS[0:5], WORDS[5:8], WORDS[8:12] + WORDS[0:2], WORDS[2:3]]
TARGET = [WORDS[3:7], WORDS[7:9], WORDS[0:3], WORDS[9:12]]
CLASSES = [[WORDS[0]], [WORDS[1]], [WORDS[0]], [WORDS[2]]]


def _vocab():
    from neuralmonkey_amd.vocabulary import Vocabulary
    return Vocabulary(WORDS)


def _decoder(name, states, final, cell):
    from neuralmonkey_amd.attention import Attention
    from neuralmonkey_amd.decoders import Decoder
    att = Attention(name="attention_" + name, encoder=states)
    dec = Decoder(encoders=[final], vocabulary=_vocab(), data_id="target", name=name, max_output_len=6,
                  embedding_size=8, rnn_size=8, attentions=[att], rnn_cell=cell)
    return att, dec


def _dataset():
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    return Dataset("four", {"source": SOURCE, "target": TARGET, "cls": CLASSES}, BatchingScheme(batch_size=4))


def _encoder():
    from neuralmonkey_amd.encoders import SentenceEncoder
    from neuralmonkey_amd.runtime import reset_registry
    reset_registry()
    return SentenceEncoder(name="encoder", vocabulary=_vocab(), data_id="source", embedding_size=8, rnn_size=8)


def _session(dev, seed=5):
    from neuralmonkey_amd.tf_manager import TensorFlowManager
    tfm = TensorFlowManager(num_sessions=1, num_threads=1, device=str(dev), seed=seed)
    tfm.initialize_sessions()
    return tfm, tfm.sessions[0]


def _snapshot(tensors):
    return {n: t.detach().cpu().numpy().copy() for n, t in tensors.items()}


def _only_through_views(dev, cell, delayed):
    from neuralmonkey_amd import tf_shim
    from neuralmonkey_amd.model.gradient_blocking import StatefulView, TemporalStatefulView
    from neuralmonkey_amd.trainers import CrossEntropyTrainer, DelayedUpdateTrainer
    from neuralmonkey_amd.trainers.objective import CostObjective
    if cell == "transformer":            # a model whose whole training step is captured and replayed as one graph
        from neuralmonkey_amd.decoders import Classifier
        from neuralmonkey_amd.encoders.transformer import TransformerEncoder
        from neuralmonkey_amd.model.sequence import EmbeddedSequence
        from neuralmonkey_amd.runtime import reset_registry
        reset_registry()
        seq = EmbeddedSequence("encoder_input", _vocab(), "source", 8)
        enc = TransformerEncoder("encoder", seq, ff_hidden_size=16, depth=1, n_heads=2)
        head = lambda name, part: Classifier(name=name, encoders=[part], vocabulary=_vocab(), data_id="cls", layers=[6],
                                             dropout_keep_prob=1.0)
        direct, blocked = head("direct", enc), head("blocked", StatefulView(enc))
    else:
        enc = _encoder()
        _, direct = _decoder("direct", enc, enc, cell)
        _, blocked = _decoder("blocked", TemporalStatefulView(enc), StatefulView(enc), cell)
    adam =lambda: tf_shim.train.AdamOptimizer(learning_rate=0.01)
    first = CrossEntropyTrainer(decoders=[direct], l2_weight=0.0, clip_norm=None, optimizer=adam())
    if delayed:
        second = DelayedUpdateTrainer(batches_per_update=2, objectives=[CostObjective(blocked)], l2_weight=0.0,
                                      optimizer=adam())
    else:
        second = CrossEntropyTrainer(decoders=[blocked], l2_weight=0.0, clip_norm=None, optimizer=adam())
    tfm, sess = _session(dev)
    store, ds = sess.store, _dataset()
    mine = [n for n in store.names() if n.startswith("encoder")]
    assert len(mine) >= 5 and "encoder_input/embedding_matrix_0" in mine
    # a direct step first: the encoder's slices of the flat gradient (and of the first trainer's slots) are not zero
    tfm.execute(ds, first.feedables, [first], train=True)
    sess.settle_training()
    assert sum(float(store.g(n).abs().max()) > 0 for n in mine) >= 5
    before = _snapshot({n: store[n] for n in store.names()})
    updates = 3
    for _ in range(updates * (2 if delayed else 1)):
        res = tfm.execute(ds, second.feedables, [second], train=True)[0]
        assert np.isfinite(float(res.losses["blocked - cost"]))
        # nobody wrote the encoder's slices in this step: zero, not the direct step's values
        assert all(not store.g(n).any() for n in mine)
    sess.settle_training()
    assert sess.global_step == 1 + updates
    after = _snapshot({n: store[n] for n in store.names()})
    for n in mine:
        assert np.array_equal(before[n], after[n]), n
    state = second._adam[id(store)]                                 # pylint: disable=protected-access
    for slot in (state["m"], state["v"]):                          # this trainer's own slots: untouched at the encoder
        for n in mine:
            spec = store.specs[n]
            assert not slot[spec.offset:spec.offset + spec.size].any(), n
    moved = [n for n in store.names() if n.startswith(("blocked", "attention_blocked"))]
    assert moved and all(not np.array_equal(before[n], after[n]) for n in moved if "bias" not in n)
    assert all(np.array_equal(before[n], after[n]) for n in store.names() if n.startswith(("direct", "attention_direct")))
    if delayed:
        accum = sess.buffer((id(second), "gradient_buffer"), (store.total,))
        for n in mine:
            spec = store.specs[n]
            assert not accum[spec.offset:spec.offset + spec.size].any(), n
    return sess


@pytest.mark.parametrize("cell", ["GRU", "LSTM", "transformer"])
def test_an_encoder_read_only_through_blocking_views_stays_as_it_is(dev, cell):
    """(a) on the hand-scheduled path (GRU), on the taped one (LSTM), and with a Transformer encoder under a Classifier,
    whose second step is captured as a graph and whose third replays it: the gradient buffer is cleared outside the
    capture, on every step."""
    sess = _only_through_views(dev, cell, delayed=False)
    replayed = sum(1 for st in sess.__dict__.get("_step_graphs", {}).values() if st[0] == 2)
    assert replayed == (1 if cell == "transformer" and sess.use_step_graphs and sess.use_graphs else 0)


def test_an_encoder_behind_blocking_views_under_delayed_updates(dev):
    """(c) three updates of two batches each."""
    _only_through_views(dev, "GRU", delayed=True)


def _data_parallel_worker(rank, port):
    """One rank under the data-parallel machinery (RCCL process group of one, sharded optimizer): every bucket of the
    flat gradient is exchanged, the encoder's zeros included."""
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      NM_DIST_FORCE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", NM_DIST_ALLREDUCE="torch", NM_DP_SHARDED="1")
    os.environ.pop("NM_DIST_BACKEND", None)
    from neuralmonkey_amd import distributed
    dp = distributed.init_from_env()
    assert dp is not None and dp.forced and dp.sharded_active()
    reduced = []
    real = dp._reduce_bucket                                        # pylint: disable=protected-access
    dp._reduce_bucket = lambda grad, plan, idx: (reduced.append(plan.buckets[idx][:2]), real(grad, plan, idx))[1]
    sess = _only_through_views(torch.device("cuda:0"), "GRU", delayed=False)
    assert sum(hi - lo for lo, hi in reduced) == 4 * sess.store.ensure_grad().numel()       # four steps, all of it
    distributed.shutdown()


def test_an_encoder_behind_blocking_views_under_data_parallelism(dev):
    """(a) once more with the gradient exchange and the sharded update of distributed.DataParallel in the step."""
    import torch.multiprocessing as mp
    from .test_dp_gpu import _free_port
    mp.spawn(_data_parallel_worker, args=(_free_port(),), nprocs=1, join=True)


def test_a_blocking_view_beside_a_direct_reader_changes_nothing(dev):
    """(b) decoder over the encoder, a Classifier over a StatefulView of it: the encoder's gradient is the one of the model
    without the classifier, bit for bit; the classifier itself learns."""
    from neuralmonkey_amd.decoders import Classifier
    from neuralmonkey_amd.model.gradient_blocking import StatefulView
    from neuralmonkey_amd.trainers import CrossEntropyTrainer
    grads, values = {}, None
    for second_head in (False, True):
        enc = _encoder()
        _, dec = _decoder("decoder", enc, enc, "GRU")
        decoders = [dec]
        if second_head:
            decoders.append(Classifier(name="classifier", encoders=[StatefulView(enc)], vocabulary=_vocab(),
                                       data_id="cls", layers=[], dropout_keep_prob=1.0))
        trainer = CrossEntropyTrainer(decoders=decoders, l2_weight=0.0, clip_norm=None)
        tfm, sess = _session(dev)
        store = sess.store
        if values is None:
            values = store.state_dict()
        else:
            store.load_state_dict(values, strict=False)
        res = tfm.execute(_dataset(), trainer.feedables, [trainer], train=True)[0]
        assert np.isfinite(float(res.losses["decoder - cost"]))
        sess.settle_training()
        grads[second_head] = _snapshot({n: store.g(n) for n in store.names()})
    alone, both = grads[False], grads[True]
    behind = [n for n in alone if n.startswith("encoder")]
    assert len(behind) >= 5
    # (the decoder's own embedding gradient is left out: its scatter-add sums the four <s> rows with float atomics)
    for n in behind:
        assert np.array_equal(alone[n], both[n]), n
    assert all(float(np.abs(alone[n]).max()) > 0 for n in behind)
    head = [n for n in both if n.startswith("classifier/")]
    assert head and all(float(np.abs(both[n]).max()) > 0 for n in head)


# ---- the non-autoregressive model ---------------------------------------------------------------------------------------------
NAT_INI = """
[main]
name="non-autoregressive"
tf_manager=<tf_manager>
output="{root}/out"
overwrite_output_dir=True
batch_size=4
epochs=1
train_dataset=<train_data>
val_dataset=<train_data>
trainer=<trainer>
runners=[<runner>]
evaluation=[("target", evaluators.BLEU)]
logging_period=1
validation_period=5
random_seed=123485

[tf_manager]
class=tf_manager.TensorFlowManager
num_threads=4
num_sessions=1

[train_data]
class=dataset.load
series=["source", "target"]
data=["{root}/source.txt", "{root}/target.txt"]

[vocabulary]
class=vocabulary.from_wordlist
path="{root}/words.vocab"
contains_header=False
contains_frequencies=False

[encoder_input]
class=model.sequence.EmbeddedSequence
name="encoder_input"
embedding_size=16
data_id="source"
vocabulary=<vocabulary>

[encoder]
class=encoders.transformer.TransformerEncoder
name="encoder"
input_sequence=<encoder_input>
ff_hidden_size=32
depth=1
n_heads=2

[splitter]
class=model.sequence_split.SequenceSplitter
name="splitter"
parent=<encoder>
factor=2
projection_size=32
projection_activation=tf.nn.relu

[encoder2]
class=encoders.transformer.TransformerEncoder
name="encoder2"
input_sequence=<splitter>
ff_hidden_size=32
depth=1
n_heads=2

[decoder]
class=decoders.ctc_decoder.CTCDecoder
name="decoder"
encoder=<encoder2>
vocabulary=<vocabulary>
data_id="target"

[trainer]
class=trainers.cross_entropy_trainer.CrossEntropyTrainer
decoders=[<decoder>]
optimizer=<optimizer>

[optimizer]
class=tf.train.AdamOptimizer
learning_rate=0.01

[runner]
class=runners.PlainRunner
decoder=<decoder>
output_series="target"
"""
NAT_SOURCE = [WORDS[0:6], WORDS[6:10], WORDS[3:6], WORDS[11:12]]
NAT_TARGET = [s + [WORDS[(WORDS.index(s[-1]) + 5) % 12]] for s in NAT_SOURCE]        # one word more than the source


def test_non_autoregressive_model_trains_through_the_config_loader(dev, tmp_path):
    from neuralmonkey_amd.config.configuration import load_experiment
    from neuralmonkey_amd.decoders.ctc_decoder import CTCDecoder
    from neuralmonkey_amd.encoders.transformer import TransformerEncoder
    from neuralmonkey_amd.model.sequence_split import SequenceSplitter
    assert max(len(s) for s in NAT_SOURCE) <= 6 and max(len(t) for t in NAT_TARGET) <= 8
    (tmp_path / "words.vocab").write_text("".join(w + "\n" for w in WORDS))
    (tmp_path / "source.txt").write_text("".join(" ".join(s) + "\n" for s in NAT_SOURCE))
    (tmp_path / "target.txt").write_text("".join(" ".join(t) + "\n" for t in NAT_TARGET))
    path = tmp_path / "nat.ini"
    path.write_text(NAT_INI.format(root=tmp_path))
    model = load_experiment(str(path), device=str(dev), seed=1234)
    dec = model.runners[0].decoder
    second = dec.encoder
    split = second.input_sequence
    assert isinstance(dec, CTCDecoder) and isinstance(second, TransformerEncoder) and isinstance(split, SequenceSplitter)
    assert isinstance(split.parent, TransformerEncoder) and (split.dimension, second.dimension) == (16, 16)
    tfm, trainer = model.tf_manager, model.trainers[0]
    sess = tfm.sessions[0]
    store = sess.store
    assert tuple(store["splitter/dense/kernel"].shape) == (16, 32) and tuple(store["splitter/dense/bias"].shape) == (32,)
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    assert split in feedables and split.parent in feedables
    ds = next(iter(model.train_dataset.batches()))
    assert len(ds) == 4
    before = _snapshot({n: store[n] for n in ("splitter/dense/kernel", "splitter/dense/bias")})
    losses = []
    for _ in range(30):
        res = tfm.execute(ds, feedables, [trainer], train=True)[0]
        losses.append(float(res.losses["decoder - cost"]))
    print("CTC cost {:.4f} -> {:.4f}".format(losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    for n, old in before.items():
        assert not np.array_equal(old, store[n].cpu().numpy()), n
    out, = tfm.execute(ds, feedables, model.runners, compute_losses=True)
    decoded = out.outputs["target"]
    assert len(decoded) == 4
    for sent, src in zip(decoded, ds.get_series("source")):
        assert len(sent) <= 2 * len(src)
    assert np.isfinite(list(out.losses.values())).all()


# ---- tests/language-model.ini -----------------------------------------------------------------------------------------------
def test_language_model_ini_verbatim_on_the_device(dev, lm_root):          # noqa: F811
    from neuralmonkey_amd.dataset import BatchingScheme
    from neuralmonkey_amd.runners import XentRunner
    from neuralmonkey_amd.vocabulary import SPECIAL_TOKENS
    from .test_reference_inis import load_verbatim
    with pytest.warns(UserWarning, match="evaluators.PerplexityEvaluator"):
        model = load_verbatim(lm_root, "language-model", device=str(dev))
    tfm = model.tf_manager
    store = tfm.sessions[0].store
    words, rows = sample_rows(lm_root)
    want = np.zeros((4 + len(words) - 2, 5), np.float64)
    at = 4
    for word, row in zip(words, rows):
        if word in SPECIAL_TOKENS:
            want[SPECIAL_TOKENS.index(word)] = row
        else:
            want[at] = row
            at += 1
    table = store["decoder/word_embeddings"].cpu().numpy()
    assert table.dtype == np.float32 and np.array_equal(table, want.astype(np.float32))
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    costs, steps = [], 0
    for batch in model.train_dataset.batches(BatchingScheme(batch_size=16)):
        res = tfm.execute(batch, feedables, model.trainers, train=True)[0]
        costs.append(float(res.losses["decoder - cost"]))
        steps += 1
        if steps == 3:
            break
    assert steps == 3 and tfm.sessions[0].global_step == 3 and np.isfinite(costs).all()
    assert not np.array_equal(store["decoder/word_embeddings"].cpu().numpy(), table)       # the embeddings train
    runner, = model.runners
    assert isinstance(runner, XentRunner)
    val = next(model.val_dataset.batches(BatchingScheme(batch_size=10)))
    out, = tfm.execute(val, feedables, model.runners, compute_losses=True)
    xents = np.asarray(out.outputs["xents"], np.float64)
    assert xents.shape[0] == 10 and np.isfinite(xents).all() and (xents > 0).all()
    assert np.isfinite(list(out.losses.values())).all()
