"""Momentum (one slot) and RMSProp (two) under data parallelism, one forced rank over RCCL as
tests/test_dp_gpu.py::test_rccl_process_group_of_one_trains_like_no_process_group launches it: the sharded optimizer
(reduce-scatter, update of the rank's chunk list, all-gather) ends bit for bit where the replicated one ends, slots
included, and a checkpoint written from the sharded run holds every slot complete.

The three updates go through the trainer (``_apply_gradients``: optimizer object -> kind and scalars -> slots ->
DataParallel.optimizer_step -> nm_optim_update / nm_optim_update_list) on gradients drawn from a seeded generator, not
through a forward and backward pass: the model's embedding gradients are scattered with float atomics, so no two runs
of a real step add them in the same order (tests/test_dp_gpu.py compares such runs to rounding only), and bit equality
is the point here."""
import os
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

LAUNCH_SECONDS = 150


def _optimizers():
    from neuralmonkey_amd.optimizers import MomentumOptimizer, RMSPropOptimizer
    return {"momentum": MomentumOptimizer(0.05, 0.9, use_nesterov=True),
            "rmsprop": RMSPropOptimizer(0.01, decay=0.9, momentum=0.5, name="rms")}


def _worker(rank, world, port, out_dir, sharded):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      NM_DIST_FORCE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", NM_DIST_ALLREDUCE="torch",
                      NM_DP_SHARDED="1" if sharded else "0", NM_DP_BIG_VARIABLE="1500")
    os.environ.pop("NM_DIST_BACKEND", None)             # default on a GPU box: nccl = RCCL
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from neuralmonkey_amd import distributed, tf_bundle
    from neuralmonkey_amd.runtime import RunContext
    from neuralmonkey_amd.trainers import CrossEntropyTrainer
    from tests.test_dp_gpu import _model
    dp = distributed.init_from_env()
    assert dp is not None and dp.world_size == 1 and dp.forced and dp.sharded_active() == bool(sharded)
    dp.bucket_elems = 1001                              # several buckets per matrix, with indivisible tails
    out = {}
    for tag, opt in _optimizers().items():
        model = _model()
        tfm = model.tf_manager
        sess = tfm.sessions[0]
        store = sess.store
        dp.broadcast_parameters(store)
        trainer = CrossEntropyTrainer(decoders=[model.decoder], l2_weight=1e-4, clip_norm=1.0, optimizer=opt)
        grad = store.ensure_grad()
        for step in range(1, 4):
            gen = torch.Generator().manual_seed(100 * step)
            # (step 2: large gradients, the clip bites on every tensor; steps 1 and 3: on some)
            grad.copy_((torch.randn(store.total, generator=gen) * (0.02 if step != 2 else 0.4)).to(grad.device))
            dp.begin_step()
            trainer._apply_gradients(RunContext(sess, {}))                         # pylint: disable=protected-access
        torch.cuda.synchronize()
        assert sess.global_step == 3 and len(store.slots()) == len(opt.slot_suffixes)
        assert dp.exchange_report()["optimizer"] == ("sharded" if sharded else "replicated")
        out[tag + "_theta"] = store.theta.cpu().numpy()
        if sharded:
            tfm.checkpoint_format = "tf"
            prefix = os.path.join(out_dir, tag + ".data")
            tfm.save(prefix)                            # (gathers the slots first: tf_manager.save)
            bundle = tf_bundle.read_bundle(prefix)
            assert not any(k.endswith("/Adam") for k in bundle) and "beta1_power" not in bundle
            for i, suffix in enumerate(opt.slot_suffixes):
                flat = np.zeros(store.total, np.float32)
                for name in store.trainable_names():
                    spec = store.specs[name]
                    flat[spec.offset:spec.offset + spec.size] = np.asarray(bundle[name + suffix]).reshape(-1)
                out["{}_ckpt{}".format(tag, i)] = flat
            assert (opt.slot_suffixes[0] + "_1" in {k[k.rfind("/"):] for k in bundle}) == (len(opt.slot_suffixes) == 2)
        for i, slot in enumerate(store.slots()):
            out["{}_slot{}".format(tag, i)] = slot.cpu().numpy()
        out[tag + "_mask"] = np.zeros(store.total, bool)
        for name in store.trainable_names():
            spec = store.specs[name]
            out[tag + "_mask"][spec.offset:spec.offset + spec.size] = True
    np.savez(os.path.join(out_dir, "sharded{}.npz".format(int(sharded))), **out)
    distributed.shutdown()


def _launch(tmp_path, sharded):
    """One forced rank in a process of its own, under its own time limit; a failure or a time-out ends the test."""
    from .test_dp_gpu import _free_port
    ctx = mp.spawn(_worker, args=(1, _free_port(), str(tmp_path), sharded), nprocs=1, join=False)
    deadline = time.monotonic() + LAUNCH_SECONDS
    while not ctx.join(timeout=1.0):                    # (raises when the worker failed)
        if time.monotonic() > deadline:
            for proc in ctx.processes:
                proc.kill()
            pytest.fail("the data-parallel worker (sharded={}) did not finish in {} s".format(sharded, LAUNCH_SECONDS))
    return dict(np.load(tmp_path / "sharded{}.npz".format(int(sharded))))


def test_sharded_update_is_the_replicated_one_bit_for_bit(tmp_path):
    replicated = _launch(tmp_path, False)
    sharded = _launch(tmp_path, True)                   # (not reached when the first launch failed)
    for tag, opt in _optimizers().items():
        nslots = len(opt.slot_suffixes)
        assert np.isfinite(sharded[tag + "_theta"]).all()
        assert np.array_equal(sharded[tag + "_theta"], replicated[tag + "_theta"]), tag
        mask = sharded[tag + "_mask"]
        for i in range(nslots):
            got, want = sharded["{}_slot{}".format(tag, i)], replicated["{}_slot{}".format(tag, i)]
            assert np.array_equal(got, want), (tag, i)
            assert not np.array_equal(want[mask], np.full(int(mask.sum()), opt.slot_initial[i], np.float32))
            # the checkpoint of the sharded run: every trainable variable's slot, complete
            assert np.array_equal(sharded["{}_ckpt{}".format(tag, i)][mask], want[mask]), (tag, i)
        assert "{}_slot{}".format(tag, nslots) not in sharded and "{}_ckpt{}".format(tag, nslots) not in sharded
    # the two optimizers did move the variables, and differently
    assert not np.array_equal(sharded["momentum_theta"], sharded["rmsprop_theta"])
