"""The batch-norm image encoder and the CTC head under data parallelism, after the pattern of tests/test_dp_gpu.py: two
ranks on ONE GPU over gloo train each model for two steps on their shards of a batch, and one process then trains on the
whole batch.  The image model (tests/cnn2d_models.build: a convolution, a max pool, a residual block with
project_input, a Classifier over the pooled map, batch norm everywhere) gets 5 images -- shards of 3 and 2, so the ranks'
row counts differ in every batch-norm layer; the CTC model (the ``speech`` experiment of tests/ctc_models.py) gets 7
sentences, 4 + 3.  Both go through the same pair of workers.

Held: the replicas end bit-identical, the moving statistics (which no optimizer touches) included; the gradient of
step 1 summed over the ranks is the one-process gradient of the whole batch, and the moving statistics' step is the
one-process step, to 2e-4 of the largest element (the rule and margin of test_dp_gpu.py); the CTC gradient is not the
full-batch gradient divided by the number of ranks."""
import datetime
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from .test_dp_gpu import _free_port

pytestmark = pytest.mark.gpu

IMAGE_CFG = dict(convolutions=[["C", 3, 1, "same", 4], ["M", 2, 2, "same"], ["R", 3, 6]], height=8, width=12,
                 pixel_dim=3, fully_connected=None, batch_normalize=True, head="classifier", cls_vocab=5, layers=[6],
                 rnn_size=5)
IMAGES, SENTENCES, STEPS = 5, 7, 2
MARGIN = 2e-4                                    # test_dp_gpu.py:127-130


# ---- the two models: -> (tf_manager, trainer, store, the whole batch) ---------------------------------------------------
def _image_model(device, root):
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    from . import cnn2d_models
    m = cnn2d_models.build(device, IMAGE_CFG)
    rng = np.random.default_rng(11)
    images = [rng.uniform(1.0, 255.0, (8, 12, 3)).astype(np.float32) for _ in range(IMAGES)]
    images[1][:, 8:] = 0.0                                              # the right third blank: the mask is not all ones
    batch = Dataset("images", {"images": images, "target": [["w{}".format(i % 5)] for i in range(IMAGES)]},
                    BatchingScheme(batch_size=IMAGES))
    return m["tfm"], m["trainer"], m["store"], batch


def _ctc_model(device, root):
    from pathlib import Path
    from . import ctc_models
    path = Path(root) / "ctc"
    path.mkdir(parents=True, exist_ok=True)
    model, _ = ctc_models.load(path, "speech", device, keep=1.0)
    batch = next(iter(model.train_dataset.batches())).subset(0, SENTENCES)
    return model.tf_manager, model.trainers[0], model.tf_manager.sessions[0].store, batch


MODELS = {"image": _image_model, "ctc": _ctc_model}


def _frozen(store):
    """Mask over the flat buffers of the variables no optimizer touches: the moving statistics."""
    mask = np.zeros(store.total, bool)
    for name in sorted(set(store.names()) - set(store.trainable_names())):
        mask[store.offset(name):store.offset(name) + store[name].numel()] = True
    return mask


def _train(tfm, trainer, store, batch):
    """STEPS steps -> theta before, after step 1 and after the last step, and the gradient buffer after step 1."""
    out = {"theta0": store.theta.cpu().numpy().copy()}
    for step in range(STEPS):
        tfm.execute(batch, trainer.feedables, [trainer], train=True)
        if step == 0:
            out["grad1"] = store.ensure_grad().cpu().numpy().copy()
            out["theta1"] = store.theta.cpu().numpy().copy()
    torch.cuda.synchronize()
    out["theta"] = store.theta.cpu().numpy().copy()
    assert np.isfinite(out["theta"]).all() and np.isfinite(out["grad1"]).all()
    out["frozen"] = _frozen(store)
    return out


def _worker(rank, world, port, out_dir, backend, kinds, forced):
    """backend gloo: all ranks share GPU 0; backend nccl (= RCCL): rank r owns GPU r."""
    local = rank if backend == "nccl" else 0
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(local), NM_DIST_BACKEND=backend, HSA_ENABLE_IPC_MODE_LEGACY="0",
                      NM_DP_BIG_VARIABLE="1500")
    if forced:
        os.environ["NM_DIST_FORCE"] = "1"
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    from neuralmonkey_amd import distributed
    torch.cuda.set_device(local)
    # the group is made here, with a short timeout: a rank that dies cannot leave its peer waiting
    dist.init_process_group(backend, timeout=datetime.timedelta(seconds=60))
    dp = distributed.init_from_env()
    assert dp is not None and dp.world_size == world and dp.forced == forced and dist.get_backend() == backend
    assert dp.sharded_active()
    dp.bucket_elems = 1001                          # several buckets, with indivisible tails
    exchanges = {"gather_parts": 0, "sum_small": 0}
    for name in exchanges:
        def spy(*args, _real=getattr(dp, name), _name=name):
            exchanges[_name] += 1
            return _real(*args)
        setattr(dp, name, spy)
    for kind in kinds:
        before = dict(exchanges)
        # (a directory per rank: the CTC experiment writes its data files before it loads them)
        tfm, trainer, store, batch = MODELS[kind]("cuda:{}".format(local), os.path.join(out_dir, "rank{}".format(rank)))
        if rank == 1:
            store.theta.add_(0.5)                   # replicas start from rank 0's variables
        dp.broadcast_parameters(store)
        shard = dp.shard(batch)
        assert len(shard) == len(batch) // world + (1 if rank < len(batch) % world else 0)
        out = _train(tfm, trainer, store, shard)
        owned = np.zeros(store.total, bool)         # sharded optimizer: a rank's gradient is the sum on its own slices
        plan = dp.plan(store)
        for lo, hi in plan.owned(rank) + plan.tails():
            owned[lo:hi] = True
        done = {k: exchanges[k] - before[k] for k in exchanges}
        # four batch-norm layers: one gather forward and one sum backward per layer and step; none for the CTC model
        assert done == ({"gather_parts": 4 * STEPS, "sum_small": 4 * STEPS} if kind == "image" else
                        {"gather_parts": 0, "sum_small": 0}), done
        np.savez(os.path.join(out_dir, "{}_rank{}.npz".format(kind, rank)), owned=owned, rows=len(shard), **out)
    distributed.shutdown()


def _one_process(kind, root, start):
    """The reference point: no process group, the whole batch, from the variables the replicas started from (an
    experiment built from INI text draws its initial values unseeded)."""
    tfm, trainer, store, batch = MODELS[kind]("cuda:0", root)
    assert store.theta.numel() == start.size
    store.theta.copy_(torch.from_numpy(start))
    store.epoch += 1                                # (the variables were written from outside)
    return _train(tfm, trainer, store, batch)


def _ranks_against_one_process(tmp_path, world, backend):
    kinds = ("image", "ctc")
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), backend, kinds, False), nprocs=world, join=True)
    for kind in kinds:
        ranks = [dict(np.load(tmp_path / "{}_rank{}.npz".format(kind, r))) for r in range(world)]
        r0 = ranks[0]
        frozen = r0["frozen"]
        assert bool(frozen.any()) == (kind == "image")
        rows = [int(r["rows"]) for r in ranks]
        assert sum(rows) == (IMAGES if kind == "image" else SENTENCES) and (world != 2 or rows[0] == rows[1] + 1)
        for other in ranks[1:]:
            assert np.array_equal(r0["theta0"], other["theta0"]), kind
            assert np.array_equal(r0["theta"][frozen], other["theta"][frozen]), kind + ": moving statistics diverged"
            assert np.array_equal(r0["theta1"], other["theta1"]) and np.array_equal(r0["theta"], other["theta"]), \
                kind + ": replicas diverged"
        # the summed gradient of step 1, from the slices their owners hold
        assert np.all(sum(r["owned"].astype(int) for r in ranks) >= 1)
        grad1 = np.zeros_like(r0["grad1"])
        for r in reversed(ranks):
            grad1[r["owned"]] = r["grad1"][r["owned"]]
        want = _one_process(kind, tmp_path / "one", r0["theta0"])
        assert np.array_equal(want["theta0"], r0["theta0"]) and np.array_equal(want["frozen"], frozen)
        scale = np.abs(want["grad1"]).max()
        err = np.abs(grad1 - want["grad1"]).max()
        ratio = np.linalg.norm(grad1.astype(np.float64)) / np.linalg.norm(want["grad1"].astype(np.float64))
        print("{} over {} {} ranks: gradient max |diff| {:.3e} = {:.3e} of max |grad| {:.3e}; norm ratio {:.6f}".format(
            kind, world, backend, err, err / scale, scale, ratio))
        assert scale > 0 and err <= MARGIN * scale, (kind, err, scale)
        assert not grad1[frozen].any() and not want["grad1"][frozen].any()
        assert abs(ratio - 1.0) <= 0.01, (kind, ratio)          # (a CTC gradient halved by a count over the ranks: 0.5)
        assert np.abs(want["theta"] - want["theta0"]).max() > 1e-5
        if kind == "image":
            step_one = want["theta1"][frozen] - want["theta0"][frozen]
            step_dp = r0["theta1"][frozen] - r0["theta0"][frozen]
            moved, off = np.abs(step_one).max(), np.abs(step_dp - step_one).max()
            print("image over {} {} ranks: moving statistics' step max |diff| {:.3e} = {:.3e} of max |step| {:.3e}".format(
                world, backend, off, off / moved, moved))
            assert moved > 1e-4 and off <= MARGIN * moved, (off, moved)
            assert np.abs(r0["theta"][frozen] - r0["theta1"][frozen]).max() > 1e-5          # ... and a second step


def test_two_ranks_equal_one_process_on_the_full_batch(tmp_path):
    (tmp_path / "one").mkdir()
    _ranks_against_one_process(tmp_path, 2, "gloo")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: one RCCL rank per GPU")
def test_two_ranks_over_rccl_equal_one_process_on_the_full_batch(tmp_path):
    """The same identities with the exchanges on RCCL, one rank per GPU."""
    (tmp_path / "one").mkdir()
    _ranks_against_one_process(tmp_path, 2, "nccl")


@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_forced_group_of_one_rank_trains_the_image_model_like_no_process_group(tmp_path, backend):
    """NM_DIST_FORCE=1: the cross-rank batch norm with a single part (every exchange the identity) is bit-equal to
    nm_bn2d_fwd / nm_bn2d_bwd, so two steps end bit for bit where a run without a process group ends.  ``nccl``: the
    two exchanges as RCCL collectives enqueued behind the stream (one GPU is enough for a group of one)."""
    (tmp_path / "one").mkdir()
    mp.spawn(_worker, args=(1, _free_port(), str(tmp_path), backend, ("image",), True), nprocs=1, join=True)
    got = np.load(tmp_path / "image_rank0.npz")
    want = _one_process("image", tmp_path / "one", got["theta0"])
    assert np.array_equal(got["theta0"], want["theta0"]) and int(got["rows"]) == IMAGES
    assert np.array_equal(got["grad1"], want["grad1"])
    assert np.array_equal(got["theta1"], want["theta1"]) and np.array_equal(got["theta"], want["theta"])
    assert bool(got["frozen"].any()) and np.abs(want["theta"][got["frozen"]] - want["theta0"][got["frozen"]]).max() > 1e-4
