"""The clip + update kernels of GradientDescent, Momentum (plain and Nesterov), Adagrad and RMSProp
(include/nmhip_optim.h, kinds 2..5 of csrc/nm_optim.hip's update kernel): called directly over the flat buffers of
tests/test_pointwise_kernels_gpu.py against the float64 restatement (tests/optim_ref.py), and behind the trainer against
the oracle's gradients plus the restatement, with a checkpoint round trip.  tests/test_optim_family_host.py shows on the
CPU that a float32 evaluation of the restatement meets the direct test's bound on the same inputs."""
import numpy as np
import pytest
import torch

from oracle import torch_ref as TR
from tests import optim_family_cases as OC
from tests import optim_ref as R

pytestmark = pytest.mark.gpu


def _passes(tables, d, kind, params, path, skip=None):
    """Regulariser terms + norms, then the update of ``kind``, over the whole table, over two ranges in reversed
    order, or over a shuffled chunk list; a slot the kind does not have is passed as NULL."""
    from .test_pointwise_kernels_gpu import i32
    s0 = d["s0"] if R.SLOTS[kind] >= 1 else None
    s1 = d["s1"] if R.SLOTS[kind] == 2 else None
    if path.startswith("whole"):
        tables.regularize_and_norms(d["theta"], d["grad"], OC.L1W, OC.L2W)
        tables.apply(kind, d["theta"], d["grad"], s0, s1, OC.CLIP, params, skip=skip)
    elif path == "ranges":
        cut = tables.nchunk // 2
        for rng_ in ((cut, tables.nchunk), (0, cut)):
            tables.partials(d["theta"], d["grad"], OC.L1W, OC.L2W, rng_)
        tables.segments()
        for rng_ in ((cut, tables.nchunk), (0, cut)):
            tables.apply(kind, d["theta"], d["grad"], s0, s1, OC.CLIP, params, skip=skip, chunks=rng_)
    else:
        order = np.random.default_rng(3).permutation(tables.nchunk).astype(np.int32)
        lst = i32(d["theta"].device, order)
        tables.partials(d["theta"], d["grad"], OC.L1W, OC.L2W, None, chunk_list=lst)
        tables.segments()
        tables.apply(kind, d["theta"], d["grad"], s0, s1, OC.CLIP, params, skip=skip, chunk_list=lst)


@pytest.fixture(scope="module")
def cases():
    """variant -> (specs, host inputs, float64 states after each of the two updates), computed once."""
    memo = {}

    def get(variant):
        if variant not in memo:
            from .test_pointwise_kernels_gpu import _optimizer_setup
            specs, _, host = _optimizer_setup("cpu", OC.seed_of(variant))
            host = OC.prepare(host, variant)
            memo[variant] = (specs, host, OC.expected(specs, host, variant))
        return memo[variant]
    return get


@pytest.mark.parametrize("path", OC.PATHS + ("whole-cut",))
@pytest.mark.parametrize("variant", sorted(OC.VARIANTS))
def test_family_kernels_direct(dev, cases, variant, path):
    """nm_optim_update / nm_optim_update_list behind passes 1 and 2, two consecutive updates (the second reads the
    accumulators the first wrote): regularised gradient, parameters and every slot the kind has against float64 within
    2e-5 x the tensor's largest entry; the frozen variable, the padding and the slots the kind lacks (passed as NULL)
    bit-unchanged.  ``whole-cut``: the whole table once more, cut inside w_a (``W_A_CUT``) so that two of its chunks
    start at odd element offsets and run the scalar loops from end to end."""
    from .test_pointwise_kernels_gpu import W_A_CUT, _optimizer_setup
    kind, params = OC.VARIANTS[variant]
    specs, host, want = cases(variant)
    _, tables, again = _optimizer_setup(dev, OC.seed_of(variant), cuts=W_A_CUT if path == "whole-cut" else ())
    assert tables.nchunk == (6 if path == "whole-cut" else 5) and np.array_equal(again["theta"], host["theta"])
    d = {k: torch.tensor(host[k], device=dev) for k in ("theta", "grad", "s0", "s1")}
    for step, key in enumerate(("grad", "grad2")):
        d["grad"].copy_(torch.tensor(host[key], device=dev))
        _passes(tables, d, kind, params, path)
        got = {k: v.cpu().numpy() for k, v in d.items()}
        OC.compare(specs, got, want[step], "{} {} update {}".format(variant, path, step + 1))
    covered = np.zeros(got["theta"].size, dtype=bool)
    for n, sp in specs.items():
        sl = slice(sp.offset, sp.offset + sp.size)
        covered[sl] = True
        if n == "frozen":
            assert all(np.array_equal(got[k][sl], host[k][sl]) for k in ("theta", "s0", "s1"))
        else:
            assert not np.array_equal(got["theta"][sl], host["theta"][sl])
    assert not covered.all()
    assert all(np.array_equal(got[k][~covered], host[k][~covered]) for k in ("theta", "s0", "s1"))
    assert np.array_equal(got["grad"][~covered], host["grad2"][~covered])
    if R.SLOTS[kind] < 1:
        assert np.array_equal(got["s0"], host["s0"])
    if R.SLOTS[kind] < 2:
        assert np.array_equal(got["s1"], host["s1"])


@pytest.mark.parametrize("variant", sorted(OC.VARIANTS))
def test_family_kernels_skip_word(dev, cases, variant):
    """With the skip word set to 1 nothing changes, on any of the three paths; with 0 the same launch updates."""
    from .test_pointwise_kernels_gpu import _optimizer_setup
    kind, params = OC.VARIANTS[variant]
    _, host, _ = cases(variant)
    _, tables, _ = _optimizer_setup(dev, OC.seed_of(variant))
    d = {k: torch.tensor(host[k], device=dev) for k in ("theta", "grad", "s0", "s1")}
    word = torch.ones(1, dtype=torch.int32, device=dev)
    for path in OC.PATHS:
        d["grad"].copy_(torch.tensor(host["grad"], device=dev))
        _passes(tables, d, kind, params, path, skip=word)
        assert all(np.array_equal(d[k].cpu().numpy(), host[k]) for k in ("theta", "s0", "s1")), path
    word.zero_()
    d["grad"].copy_(torch.tensor(host["grad"], device=dev))
    _passes(tables, d, kind, params, "lists", skip=word)
    assert not np.array_equal(d["theta"].cpu().numpy(), host["theta"])


# ---- behind the trainer -------------------------------------------------------------------------------------------------
def _trainer_cases():
    from neuralmonkey_amd.optimizers import (AdagradOptimizer, GradientDescentOptimizer, MomentumOptimizer,
                                             RMSPropOptimizer)
    # (learning rates at which four clipped steps move the loss visibly)
    return {"sgd": GradientDescentOptimizer(0.5),
            "momentum": MomentumOptimizer(0.2, 0.9, name="momentum"),
            "nesterov": MomentumOptimizer(0.2, 0.9, use_nesterov=True),
            "adagrad": AdagradOptimizer(0.05, initial_accumulator_value=0.1),
            "rmsprop": RMSPropOptimizer(0.01, decay=0.9, momentum=0.5, epsilon=1e-10, name="rms")}


@pytest.mark.parametrize("variant", ["sgd", "momentum", "nesterov", "adagrad", "rmsprop"])
def test_trainer_steps_track_the_oracle(dev, tmp_path, variant):
    """Four updates of the model of tests/test_training_gpu.py behind the trainer's clip against the oracle's gradients
    (TR.train_step_grads) plus the restatement in float64, with test_adadelta_steps_track_the_oracle's bounds: losses
    rtol 2e-4, parameters and slots within 5e-3 x max|want| per tensor, the last loss below the first by more than
    1e-3.  clip = 0.05 bites on 9..13 of the 27 tensors in every step and spares the others (counted on the
    restatement alone).  Then a TF-format checkpoint: exactly the optimizer's slot variables, and a restore puts back,
    bit for bit, the slots that were saved."""
    from neuralmonkey_amd import tf_bundle
    from neuralmonkey_amd.trainers import CrossEntropyTrainer
    from .test_training_gpu import _build
    clip, l2 = 0.05, 1e-3
    opt = _trainer_cases()[variant]
    nslots = len(opt.slot_suffixes)
    model, params, ds, src, tgt = _build(dev, 200, 32, 32, 8, 10, 9, True, l2=l2, clip=clip)
    trainer = CrossEntropyTrainer(decoders=[model.decoder], l2_weight=l2, clip_norm=clip, optimizer=opt)
    tfm = model.tf_manager
    store = tfm.sessions[0].store
    tp = TR.to_torch(params)
    slots = [{k: np.full(tuple(v.shape), value, np.float64) for k, v in tp.items()} for value in opt.slot_initial]
    slots += [None, None]
    ref_losses, got_losses = [], []
    for step in range(1, 5):
        loss, _, _, grads = TR.train_step_grads(tp, src, tgt, l1_weight=0.0, l2_weight=l2)
        ref_losses.append(float(loss))
        p = {k: v.detach().numpy().astype(np.float64) for k, v in tp.items()}
        g = {k: v.numpy().astype(np.float64) for k, v in grads.items()}
        clipped = R.clip_and_update(opt.kind, p, g, slots[0], slots[1], clip, opt.params(step))
        assert 0 < clipped < len(tp), "the clip must bite on some tensors and spare others for the test to mean anything"
        with torch.no_grad():
            for k in tp:
                tp[k].copy_(torch.from_numpy(np.asarray(p[k], np.float32)))
        res = tfm.execute(ds, trainer.feedables, [trainer], train=True)[0]
        got_losses.append(res.losses["decoder - cost"])
    print(variant, "losses", got_losses, ref_losses)
    assert np.allclose(got_losses, ref_losses, rtol=2e-4), (got_losses, ref_losses)
    assert got_losses[3] < got_losses[0] - 1e-3
    assert len(store.slots()) == nslots and (store.adam_m is None) == (nslots == 0) and (store.adam_v is None) == (nslots < 2)
    assert store.slot_suffixes == tuple(opt.slot_suffixes)
    for name in store.names():
        if name.endswith("attn_bias"):          # its gradient is identically 0: rounding noise on both sides
            continue
        spec = store.specs[name]
        sl = slice(spec.offset, spec.offset + spec.size)
        pairs = [(store[name], p[name], "variable")]
        pairs += [(slot[sl], slots[i][name], "slot{}".format(i)) for i, slot in enumerate(store.slots())]
        for got, want, what in pairs:
            got, want = got.cpu().numpy().reshape(-1), np.asarray(want).reshape(-1)
            err, bound = np.abs(got - want).max(), 5e-3 * max(np.abs(want).max(), 1e-12)
            print(variant, name, what, "err {:.3g} bound {:.3g}".format(err, bound))
            assert err <= bound, (name, what, err, bound)
    tfm.checkpoint_format = "tf"
    prefix = str(tmp_path / "variables.data")
    tfm.save(prefix)
    keys = set(tf_bundle.read_bundle(prefix))
    slotted = [n for n in store.names() if store.specs[n].trainable] + list(store.checkpoint_only)
    want_keys = set(store.names()) | set(store.checkpoint_only) | {"global_step"}
    want_keys |= {n + s for n in slotted for s in opt.slot_suffixes}
    assert keys == want_keys, keys ^ want_keys
    assert "beta1_power" not in keys and not any(k.endswith("/Adam") for k in keys)
    kept = [s.clone() for s in store.slots()]
    for s in store.slots():
        s.zero_()
    store.slot_suffixes = ("/Adam", "/Adam_1")                # a fresh process has not named the slots yet
    tfm.restore(prefix)
    assert len(store.slots()) == nslots
    for name in store.trainable_names():                      # (the padding between variables is in no checkpoint)
        spec = store.specs[name]
        sl = slice(spec.offset, spec.offset + spec.size)
        assert all(torch.equal(a[sl], b[sl]) for a, b in zip(store.slots(), kept)), name
    if nslots:
        assert store.slot_suffixes == tuple(opt.slot_suffixes)
