"""A GRU time loop launched as ONE cluster kernel (csrc/nm_gru_cluster.hip) needs all its workgroups resident at
once; when something else holds compute units its hand-offs time out, it raises the session's error word and its
results are garbage.  That must cost a slow step, not the run:

  * the optimizer kernels skip their update while the word is set (nm_optim_apply, ``skip_word``), so nothing of
    the garbage reaches the variables or the optimizer slots;
  * the session switches to the per-step path (ONE warning), runs the affected steps / batches again from their
    saved feeds and hands their losses to whoever holds the lazily-read losses of the failed runs;
  * the result equals a run in which the same steps were taken on the per-step path from the start: the loss of
    the step that is run again is bit-identical (same variables, same kernels); everything after it to rounding
    only, because the embedding gradients are scattered with float atomics (csrc/nm_backward.hip:
    embedding_scatter_kernel) and no two runs add them in the same order.  A skipped, doubled or garbage update
    would move every variable by ~learning rate = 1e-4; the tests allow a mean difference of 2e-8.

What runs between the given-up step and the read of its flag must not break that: a validation pass
(TensorFlowManager.execute(train=False) settles the training steps before it launches anything), a save
(Session.settle_training), an open accumulation window, another optimizer, a host that flushes denormals (the flag
travels as int32 bits in a float32 slot and is read as an integer) -- and the Nematus, LSTM and GRU-layer loops of the
taped path raise the same word as the fast path's.

The give-up is forced by the library's test hook (nm_gru_seq_force_give_up: the launch raises its error word at
once instead of after 0.2 s) and, once, provoked for real: 32 workgroups of another stream sit on 32 CUs with all
their LDS while a training step is launched.  Reference semantics: trainers/generic_trainer.py:179-195 (one update
per batch), decoders/autoregressive.py:313-316.
"""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VOCAB, DIM, BATCH, SLEN, TLEN = 300, 256, 24, 9, 8


def _model(dev, trainer_cls=None, **kw):
    from neuralmonkey_amd import synthetic
    from oracle import nm_oracle as O
    model = synthetic.build_translation_model(vocab_src=VOCAB, vocab_tgt=VOCAB, emb=DIM, rnn=DIM, max_len=12,
                                              beam_size=0, device=str(dev))
    params = O.init_params(seed=3, vocab_src=VOCAB, vocab_tgt=VOCAB, emb=DIM, rnn=DIM, std=0.1)
    model.tf_manager.sessions[0].store.load_state_dict(params)
    if trainer_cls is not None:
        trainer = trainer_cls(objectives=model.trainer.objectives, l2_weight=1e-8, clip_norm=1.0, **kw)
        model = model._replace(trainer=trainer)
    return model


def _batches(n):
    from neuralmonkey_amd import synthetic
    return [synthetic.synthetic_dataset(seed=10 + i, batch=BATCH, src_len=SLEN, tgt_len=TLEN, vocab=VOCAB, ragged=True)
            for i in range(n)]


def _close(losses, ref_losses, exact_at=None):
    assert len(losses) == len(ref_losses)
    for i, (got, want) in enumerate(zip(losses, ref_losses)):
        assert got.keys() == want.keys()
        for name in got:
            if i == exact_at:
                assert got[name] == want[name], "step {}: {} {} != {}".format(i, name, got[name], want[name])
            else:
                assert abs(got[name] - want[name]) <= 1e-5 * abs(want[name]), (i, name, got[name], want[name])


def _same_variables(theta, ref_theta):
    """A lost, doubled or garbage update moves EVERY element with a gradient by about the learning rate (Adam: 1e-4 per
    step); the order of the float atomics moves a few elements whose gradient nearly cancels by a few 1e-6 and the
    rest by 1e-9 or less."""
    assert torch.isfinite(theta).all()
    diff = (theta - ref_theta).abs()
    assert float(diff.mean()) < 2e-8 and float(diff.max()) < 3e-5, \
        "variables differ (mean {:.2e}, max {:.2e}): an update was lost, doubled or garbage".format(float(diff.mean()),
                                                                                                  float(diff.max()))


def _uses_cluster_loops(model):
    from neuralmonkey_amd import ops
    return model.tf_manager.sessions[0].use_cluster_loops and ops.gru_seq_supported(BATCH, DIM, 1)


def _same_slots(sess, ref_sess):
    """The optimizer's slots (Adam: m, v; Momentum: its accumulator) are the reference's: a garbage gradient that got
    through the gate would be in them for good."""
    slots, ref_slots = sess.store.slots(), ref_sess.store.slots()
    assert len(slots) == len(ref_slots) and slots
    for got, want in zip(slots, ref_slots):
        assert torch.isfinite(got).all()
        assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max()), \
            "optimizer slots differ: a garbage update got through"


def _train(model, batches, fail_before=None, stepwise_from=None, read_losses="end", between=None):
    """Training steps over ``batches``; ``fail_before`` = index of the step whose first cluster loop is forced to
    give up; ``stepwise_from`` = index from which the session is put on the per-step path by hand (the reference
    run); ``read_losses``: "each" reads every step's losses right away, "end" only after the last step, "later"
    not at all: the unread results are returned in place of the losses; ``between(i)`` runs after step ``i`` was
    enqueued (and, with "each", read)."""
    from neuralmonkey_amd import ops
    tfm = model.tf_manager
    sess = tfm.sessions[0]
    results = []
    try:
        for i, ds in enumerate(batches):
            if stepwise_from is not None and i == stepwise_from:
                torch.cuda.synchronize()
                sess.use_cluster_loops = False
                sess._graphs.clear()                                   # pylint: disable=protected-access
            if fail_before is not None and i == fail_before:
                ops.gru_seq_force_give_up(1)
            res = tfm.execute(ds, model.trainer.feedables, [model.trainer], train=True)[0]
            if read_losses == "each":
                dict(res.losses)
            results.append(res)
            if between is not None:
                between(i)
        losses = results if read_losses == "later" else [dict(r.losses) for r in results]
        torch.cuda.synchronize()
        left = ops.gru_seq_force_give_up(0)
    finally:
        ops.gru_seq_force_give_up(0)
    assert left == 0, "the forced give-up was never consumed: no cluster loop was launched"
    return losses, sess.store.theta.clone(), sess


@pytest.mark.parametrize("read_losses", ["end", "each"])
@pytest.mark.parametrize("fail_at", [0, 2])
def test_a_given_up_time_loop_costs_a_slow_step_not_the_run(dev, fail_at, read_losses):
    batches = _batches(5)
    ref_model = _model(dev)
    if not _uses_cluster_loops(ref_model):
        pytest.skip("cluster loops are off or unsupported on this device")
    ref_losses, ref_theta, ref_sess = _train(ref_model, batches, stepwise_from=fail_at, read_losses=read_losses)
    model = _model(dev)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        losses, theta, sess = _train(model, batches, fail_before=fail_at, read_losses=read_losses)
    told = [w for w in caught if "gave up waiting" in str(w.message)]
    assert len(told) == 1, "exactly one warning"
    assert not sess.use_cluster_loops and sess.cluster_demotions == 1
    assert sess.global_step == ref_sess.global_step == len(batches)
    _close(losses, ref_losses, exact_at=fail_at if fail_at == 0 else None)
    _same_variables(theta, ref_theta)
    assert not sess.cluster_failure()
    assert len(sess.store.slots()) == 2          # Adam's m and v
    _same_slots(sess, ref_sess)


def test_the_garbage_update_is_skipped_on_the_device(dev):
    """The gate itself: with the error word set by hand the optimizer launch leaves variables and slots alone."""
    model = _model(dev)
    tfm, sess = model.tf_manager, model.tf_manager.sessions[0]
    ds = _batches(1)[0]
    dict(tfm.execute(ds, model.trainer.feedables, [model.trainer], train=True)[0].losses)
    torch.cuda.synchronize()
    before = sess.store.theta.clone()
    m0 = sess.store.ensure_adam()[0].clone()
    from neuralmonkey_amd import ops
    tables = model.trainer._optim_tables(sess.store)               # pylint: disable=protected-access
    grad = sess.store.ensure_grad()
    grad.fill_(0.5)
    m, v = sess.store.ensure_adam()
    word = torch.ones(1, dtype=torch.int32, device=dev)
    tables.regularize_and_norms(sess.store.theta, grad, 0.0, 0.0)
    tables.clip_adam(sess.store.theta, grad, m, v, 1.0, 1e-3, 0.9, 0.999, 1e-8, skip=word)
    torch.cuda.synchronize()
    assert torch.equal(sess.store.theta, before) and torch.equal(m, m0)
    word.zero_()
    tables.clip_adam(sess.store.theta, grad, m, v, 1.0, 1e-3, 0.9, 0.999, 1e-8, skip=word)
    torch.cuda.synchronize()
    assert not torch.equal(sess.store.theta, before)
    ops.zero_if(word, grad)
    assert float(grad.abs().max()) > 0
    word.fill_(1)
    ops.zero_if(word, grad)
    assert float(grad.abs().max()) == 0.0


def test_delayed_updates_survive_a_given_up_loop_in_the_middle_of_a_window(dev):
    """trainers/delayed_update_trainer.py:142-204: the accumulation buffer lives across steps; the failed step's
    gradient is zeroed on the device before it is added, and the window goes on from the step that is run again."""
    from neuralmonkey_amd.trainers import DelayedUpdateTrainer
    batches = _batches(6)
    for fail_at in (1, 3):                                        # second batch of a window / first of the next
        ref_model = _model(dev, DelayedUpdateTrainer, batches_per_update=3)
        if not _uses_cluster_loops(ref_model):
            pytest.skip("cluster loops are off or unsupported on this device")
        ref_losses, ref_theta, _ = _train(ref_model, batches, stepwise_from=fail_at)
        model = _model(dev, DelayedUpdateTrainer, batches_per_update=3)
        with warnings.catch_warnings(record=True):
            warnings.simplefilter("always")
            losses, theta, sess = _train(model, batches, fail_before=fail_at)
        _close(losses, ref_losses)
        _same_variables(theta, ref_theta)
        assert sess.global_step == 2 and not sess.use_cluster_loops


def test_inference_runs_the_batch_again_on_the_per_step_path(dev):
    from neuralmonkey_amd import ops
    model = _model(dev)
    if not _uses_cluster_loops(model):
        pytest.skip("cluster loops are off or unsupported on this device")
    tfm, sess = model.tf_manager, model.tf_manager.sessions[0]
    a, b = _batches(2)
    want_a = tfm.execute(a, model.greedy_runner.feedables, [model.greedy_runner])[0].outputs["target"]
    want_b = tfm.execute(b, model.greedy_runner.feedables, [model.greedy_runner])[0].outputs["target"]
    ops.gru_seq_force_give_up(1)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got_a = tfm.execute(a, model.greedy_runner.feedables, [model.greedy_runner], lookahead=b)[0].outputs["target"]
        got_b = tfm.execute(b, model.greedy_runner.feedables, [model.greedy_runner])[0].outputs["target"]
    assert ops.gru_seq_force_give_up(0) == 0
    assert len([w for w in caught if "gave up waiting" in str(w.message)]) == 1
    assert got_a == want_a and got_b == want_b
    assert not sess.use_cluster_loops
    # a raised word with the loops already off is the fallback's own failure: that one raises
    sess.error_word().fill_(1)
    with pytest.raises(RuntimeError, match="gave up waiting"):
        tfm.execute(a, model.greedy_runner.feedables, [model.greedy_runner])
    sess.error_word().zero_()


def test_two_cluster_loops_on_two_streams_take_turns(dev):
    """One workgroup of a cluster loop fits a CU (8 waves x 160 registers): two loops launched at once on two streams
    would interleave over the CUs and both time out.  ops.gru_seq_fwd orders every launch behind the previous one's
    event, whatever its stream."""
    from neuralmonkey_amd import ops
    rows, steps, h = 48, 12, 256
    if not ops.gru_seq_supported(rows, h, 1):
        pytest.skip("cluster loops unsupported on this device")
    g = torch.Generator(device=dev).manual_seed(5)
    xp = torch.randn(rows * steps, 3 * h, device=dev, generator=g) * 0.5
    wgh = torch.randn(1, h, 2 * h, device=dev, generator=g) * 0.09
    wch = torch.randn(1, h, h, device=dev, generator=g) * 0.09
    strides = (3 * h, steps * 3 * h, 3 * h)

    def loop(ws):
        hb = torch.zeros(1, rows, h, device=dev)
        ru = torch.empty(steps, 1, rows, 2 * h, device=dev)
        cs = torch.empty(steps, 1, rows, h, device=dev)
        out = torch.zeros(rows, steps, h, device=dev)
        ops.gru_seq_fwd(steps, 1, rows, h, xp, strides, hb, hb, 0, ru[0], rows * 2 * h, None, 0, cs[0], rows * h,
                        wgh, wch, ws, out=out, out_strides=(h, steps * h, h))
        return out, hb

    ws = [ops.gru_seq_workspace(rows, h, 1, dev) for _ in range(3)]
    want, want_h = loop(ws[0])
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    outs = []
    for _ in range(4):
        with torch.cuda.stream(s1):
            outs.append((loop(ws[1]), ws[1]))
        with torch.cuda.stream(s2):
            outs.append((loop(ws[2]), ws[2]))
        torch.cuda.synchronize()
        for (out, hb), w in outs[-2:]:
            assert not ops.gru_seq_failed(w), "a cluster loop gave up: two loops were resident at once"
            assert torch.equal(out, want) and torch.equal(hb, want_h)


@pytest.mark.slow
def test_a_real_compute_unit_hog_makes_the_loop_give_up_and_the_step_is_recovered(dev):
    """Not the hook: 32 workgroups of another stream hold 32 CUs' LDS for 0.6 s while a training step is launched.
    The step's first cluster loop cannot place all its workgroups, gives up after 0.2 s, and the step is run again
    on the per-step path -- same losses and variables as a per-step run."""
    from neuralmonkey_amd import ops
    batches = _batches(3)
    ref_model = _model(dev)
    if not _uses_cluster_loops(ref_model):
        pytest.skip("cluster loops are off or unsupported on this device")
    ref_losses, ref_theta, _ = _train(ref_model, batches, stepwise_from=1)
    model = _model(dev)
    tfm, sess = model.tf_manager, model.tf_manager.sessions[0]
    side = torch.cuda.Stream(device=dev)
    losses = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for i, ds in enumerate(batches):
            if i == 1:
                torch.cuda.synchronize()
                ops.gru_seq_test_hog(32, 160 * 1024, 600000, stream=side)
            losses.append(dict(tfm.execute(ds, model.trainer.feedables, [model.trainer], train=True)[0].losses))
    torch.cuda.synchronize()
    if sess.use_cluster_loops:
        pytest.skip("the hog did not keep the loop from becoming resident on this device")
    assert len([w for w in caught if "gave up waiting" in str(w.message)]) == 1
    _close(losses, ref_losses)
    _same_variables(sess.store.theta, ref_theta)


# ---- training, validation, logging: what runs between a given-up step and the read of its losses ---------------------
def _validation_after(model, step, ds, seen):
    """A ``between`` hook for ``_train``: after training step ``step`` the greedy runner decodes ``ds`` twice in a row
    (train=False), the decoded tokens go to ``seen``."""
    tfm = model.tf_manager

    def between(i):
        if i == step:
            for _ in range(2):
                res = tfm.execute(ds, model.greedy_runner.feedables, [model.greedy_runner], train=False)[0]
                seen.append(res.outputs["target"])
    return between


def _recovered_and_reference(dev, build, batches, fail_at, validate_after, read_losses="end"):
    """The reference run (per-step path by hand from ``fail_at``) and the run whose step ``fail_at`` gives up, both
    with the same validation batch decoded after step ``validate_after``.  -> (losses, theta, sess, warnings told,
    decoded) of the recovered run and (losses, theta, sess) of the reference."""
    val = _batches(len(batches) + 1)[-1]
    ref_model = build()
    if not _uses_cluster_loops(ref_model):
        pytest.skip("cluster loops are off or unsupported on this device")
    ref = _train(ref_model, batches, stepwise_from=fail_at, read_losses=read_losses,
                 between=_validation_after(ref_model, validate_after, val, []))
    model = build()
    seen = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = _train(model, batches, fail_before=fail_at, read_losses=read_losses,
                     between=_validation_after(model, validate_after, val, seen))
    told = [w for w in caught if "gave up waiting" in str(w.message)]
    return got + (told, seen), ref


@pytest.mark.parametrize("fail_at,validate_after", [(0, 0), (2, 2), (1, 2)])
def test_a_validation_pass_before_the_losses_are_read_does_not_break_recovery(dev, fail_at, validate_after):
    """Train, validate, log: TensorFlowManager.execute(train=False) runs while the given-up step's error flag is still
    unread.  It must settle the training steps first -- not take their sticky word for its own batch's, clear it and
    leave the voided updates missing (the loss read then met a session that was demoted already and raised)."""
    (losses, theta, sess, told, seen), (ref_losses, ref_theta, ref_sess) = _recovered_and_reference(
        dev, lambda: _model(dev), _batches(5), fail_at, validate_after)
    assert len(told) == 1, "exactly one warning"
    assert not sess.use_cluster_loops and sess.cluster_demotions == 1
    assert sess.global_step == ref_sess.global_step == 5
    _close(losses, ref_losses)
    _same_variables(theta, ref_theta)
    _same_slots(sess, ref_sess)
    assert not sess.cluster_failure()
    # the same variables, both runs on the per-step path, no atomics in the forward pass
    assert len(seen) == 2 and seen[0] == seen[1]


def test_delayed_updates_survive_a_validation_pass_inside_the_window(dev):
    """As above with an accumulation window open: the failed batch's gradient was zeroed on the device, the validation
    pass settles the window before it runs and the window goes on from the batch that is run again."""
    from neuralmonkey_amd.trainers import DelayedUpdateTrainer
    (losses, theta, sess, told, _), (ref_losses, ref_theta, _) = _recovered_and_reference(
        dev, lambda: _model(dev, DelayedUpdateTrainer, batches_per_update=3), _batches(6), 1, 1)
    _close(losses, ref_losses)
    _same_variables(theta, ref_theta)
    assert sess.global_step == 2 and not sess.use_cluster_loops and len(told) == 1


def test_momentum_recovers_through_a_validation_pass_like_adam(dev):
    """The (2, 2) case with tf.train.MomentumOptimizer: one slot, no bias-correction counter.  The update is
    lr * (momentum-averaged clipped gradient) instead of Adam's ~lr per element, so the test first checks that ONE
    update moves the variables by far more than ``_same_variables`` allows two runs to differ."""
    from neuralmonkey_amd.optimizers import MomentumOptimizer
    from neuralmonkey_amd.trainers import GenericTrainer
    build = lambda: _model(dev, GenericTrainer, optimizer=MomentumOptimizer(learning_rate=0.1, momentum=0.9))
    start = build().tf_manager.sessions[0].store.theta.clone()
    (losses, theta, sess, told, seen), (ref_losses, ref_theta, ref_sess) = _recovered_and_reference(
        dev, build, _batches(5), 2, 2)
    moved = float((ref_theta - start).abs().mean()) / 5
    print("one Momentum update moves the variables by {:.3g} on average".format(moved))
    assert moved > 100 * 2e-8, "a lost update would hide inside the bound of _same_variables: raise the learning rate"
    assert len(told) == 1 and sess.cluster_demotions == 1 and not sess.use_cluster_loops
    assert sess.global_step == ref_sess.global_step == 5
    _close(losses, ref_losses)
    _same_variables(theta, ref_theta)
    assert len(sess.store.slots()) == 1          # the accumulator
    _same_slots(sess, ref_sess)
    assert not sess.cluster_failure()
    assert len(seen) == 2 and seen[0] == seen[1]


def test_saving_settles_the_outstanding_steps_first(dev, tmp_path):
    """TensorFlowManager.save -> Session.settle_training: with the last step's flag unread, saving runs that step
    again first.  The file holds the variables of three clean steps and step 3; the losses read afterwards are the
    re-run's (HostPending.redirect)."""
    batches = _batches(3)
    ref_model = _model(dev)
    if not _uses_cluster_loops(ref_model):
        pytest.skip("cluster loops are off or unsupported on this device")
    ref_losses, ref_theta, _ = _train(ref_model, batches, stepwise_from=2)
    model = _model(dev)
    path = str(tmp_path / "variables")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        results, _, sess = _train(model, batches, fail_before=2, read_losses="later")
        model.tf_manager.save(path)
        torch.cuda.synchronize()
        assert sess.global_step == 3
        assert sess.__dict__.get("_train_guard") == [], "every outstanding record was read"
        assert not sess.use_cluster_loops and sess.cluster_demotions == 1
        saved = sess.store.theta.clone()
        losses = [dict(r.losses) for r in results]
    assert len([w for w in caught if "gave up waiting" in str(w.message)]) == 1
    _same_variables(saved, ref_theta)
    assert torch.equal(sess.store.theta, saved), "reading the losses after the save changed nothing"
    _close(losses, ref_losses)
    fresh = _model(dev)
    fresh.tf_manager.restore(path)
    fresh_sess = fresh.tf_manager.sessions[0]
    assert torch.equal(fresh_sess.store.theta, saved) and fresh_sess.global_step == 3


def test_recovery_tolerates_a_session_that_was_demoted_already(dev):
    """A caller that drives inference on the session by hand sees the last training step's sticky word first and
    switches the loops off (what TensorFlowManager.execute did before it settled the training steps).  The read of
    the step's losses still runs the step again: ``recover_training`` raises only when the re-run sets the word."""
    batches = _batches(3)
    ref_model = _model(dev)
    if not _uses_cluster_loops(ref_model):
        pytest.skip("cluster loops are off or unsupported on this device")
    ref_losses, ref_theta, ref_sess = _train(ref_model, batches, stepwise_from=2)
    model = _model(dev)
    sess = model.tf_manager.sessions[0]

    def by_hand(i):
        if i == 2:
            assert sess.cluster_failure()
            sess.demote_cluster_loops()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        losses, theta, _ = _train(model, batches, fail_before=2, between=by_hand)
    assert len([w for w in caught if "gave up waiting" in str(w.message)]) == 1
    assert not sess.use_cluster_loops and sess.cluster_demotions == 1 and sess.global_step == 3
    _close(losses, ref_losses)
    _same_variables(theta, ref_theta)
    _same_slots(sess, ref_sess)
    assert not sess.cluster_failure()


def test_recovery_with_the_host_flushing_denormals(dev):
    """The error word travels behind the losses as raw int32 bits in a float32 slot: a 1 is the denormal 1.4e-45, which
    a host with flush-to-zero on reads as 0.0.  Read through an integer view (runtime.error_flag_set) the give-up is
    seen all the same; before, no warning came and the sticky word voided every later update."""
    batches = _batches(5)
    ref_model = _model(dev)
    if not _uses_cluster_loops(ref_model):
        pytest.skip("cluster loops are off or unsupported on this device")
    ref_losses, ref_theta, ref_sess = _train(ref_model, batches, stepwise_from=2)
    model = _model(dev)
    if not torch.set_flush_denormal(True):
        pytest.skip("this host cannot flush denormals")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            losses, theta, sess = _train(model, batches, fail_before=2)
    finally:
        torch.set_flush_denormal(False)
    told = [w for w in caught if "gave up waiting" in str(w.message)]
    assert len(told) == 1, "exactly one warning"
    assert not sess.use_cluster_loops and sess.cluster_demotions == 1
    assert sess.global_step == ref_sess.global_step == len(batches)
    _close(losses, ref_losses)
    _same_variables(theta, ref_theta)
    assert not sess.cluster_failure()
    assert len(sess.store.slots()) == 2
    _same_slots(sess, ref_sess)


# ---- the other loops that raise the same word: NematusGRU, LSTM and GRU layers of the taped path ---------------------
def _taped_config(cell):
    from oracle import general_ref as G
    if cell == "NematusGRU":
        return G.Config(rnn_layers=((256, "bidirectional", "NematusGRU"),), dec_cell="NematusGRU", conditional_gru=True,
                        rnn_size=8, output_projection=("nematus", "tanh", 1.0)), "nematus_seq_fwd"
    if cell == "LSTM":
        return G.Config(rnn_layers=((256, "bidirectional", "LSTM"),), dec_cell="LSTM", rnn_size=8), "lstm_seq_fwd"
    # (layer-normed: the general path, encoders/recurrent.py::_gru_cluster_layer)
    return G.Config(rnn_layers=((256, "bidirectional", "GRU"),), add_layer_norm=True, dec_cell="GRU",
                    rnn_size=8), "gru_seq_fwd"


@pytest.mark.parametrize("cell", ["NematusGRU", "LSTM", "GRU"])
def test_the_taped_path_loops_recover_like_the_fast_path(dev, cell, monkeypatch):
    """encoders/recurrent.py: the Nematus, LSTM and GRU-layer loops raise the session's word like the fast path's.
    Three Adam steps (lr 1e-4) on a 256-wide, 5-sentence model, step 1's first loop -- the encoder layer's -- gives up.

    Reference: the same model on the per-step path from the start.  A lost or doubled update moves every trained
    element by about lr; the float atomics' order moves them by orders of magnitude less.  The test checks that
    premise itself: two per-step runs differ by less than lr / 10000 on average; the recovered run must be within
    lr / 100 of the reference."""
    import types
    from neuralmonkey_amd import ops
    from tests.test_general_gpu import _build, _data
    cfg, loop = _taped_config(cell)
    lr = 1e-4
    batches = [_data(5, 7, 6, 8, seed=3 + i)[0] for i in range(3)]
    calls = []                                       # (training step, demotions so far) of every forward loop
    now = {"step": 0, "sess": None}
    real = getattr(ops, loop)

    def spy(*a, **k):
        calls.append((now["step"], getattr(now["sess"], "cluster_demotions", 0)))
        return real(*a, **k)
    monkeypatch.setattr(ops, loop, spy)

    def run(**how):
        m = _build(dev, cfg, 12, 8, init_std=0.08)
        assert type(m["trainer"].optimizer).__name__ == "AdamOptimizer" and m["trainer"].optimizer.learning_rate(1) == lr
        model = types.SimpleNamespace(tf_manager=m["tfm"], trainer=m["trainer"])
        now["step"], now["sess"] = 0, m["tfm"].sessions[0]
        del calls[:]

        def between(i):
            now["step"] = i + 1
        return _train(model, batches, read_losses="each", between=between, **how)

    ref_losses, ref_theta, _ = run(stepwise_from=0)
    assert not calls, "the reference runs no cluster loop"
    _, ref_theta2, _ = run(stepwise_from=0)
    noise = float((ref_theta2 - ref_theta).abs().mean())
    print("{}: two per-step runs differ by {:.3g} on average".format(cell, noise))
    assert noise < lr / 10000
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        losses, theta, sess = run(fail_before=1)
    assert len([w for w in caught if "gave up waiting" in str(w.message)]) == 1
    assert not sess.use_cluster_loops and sess.cluster_demotions == 1 and sess.global_step == 3
    steps = {step for step, _ in calls}
    assert 0 in steps and 1 in steps, "the layer took its loop before the failure"
    assert 2 not in steps and all(demoted == 0 for _, demoted in calls), "no loop after the failure"
    _close(losses, ref_losses)
    assert torch.isfinite(theta).all()
    diff = float((theta - ref_theta).abs().mean())
    print("{}: recovered run and reference differ by {:.3g} on average".format(cell, diff))
    assert diff < lr / 100, "variables differ: an update was lost, doubled or garbage"
