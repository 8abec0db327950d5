"""Batch norm over all ranks and the summed CTC loss under data parallelism, without a GPU: the binding table of
include/nmhip_bnsync.h (the image header and its table unchanged beside it), the refusals of its four entry points
before any launch, and -- with a stub DataParallel of two ranks made current -- the model parts' side: CTCDecoder no
longer refuses, the trainer scales a ``loss_is_batch_sum`` decoder by the objective's weight without a collective, and
a ReinforceObjective is still refused."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from . import ctc_models
from .test_cnn2d_host import ROOT, image_header_symbols


def bnsync_header_symbols():
    text = open(os.path.join(ROOT, "include", "nmhip_bnsync.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nm_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


# ---- the binding table -------------------------------------------------------------------------------------------------------
def test_bnsync_header_matches_its_binding_table(lib):
    from neuralmonkey_amd import _lib
    from .test_abi import header_symbols
    mine = bnsync_header_symbols()
    assert mine == set(_lib.BNSYNC_SIGNATURES) == {"nm_bn2d_part_stats", "nm_bn2d_merge", "nm_bn2d_bwd_sums",
                                                   "nm_bn2d_bwd_dx"}
    for name, (res, args) in _lib.BNSYNC_SIGNATURES.items():
        fn = getattr(lib, name)                                          # exported, and bound by load()
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    tables = [getattr(_lib, n) for n in dir(_lib) if n.endswith("SIGNATURES") and n != "BNSYNC_SIGNATURES"]
    assert len(tables) >= 10 and not any(mine & set(t) for t in tables)
    assert not mine & header_symbols()
    # the image header and its table are what they were
    image = image_header_symbols()
    assert image == set(_lib.IMAGE_SIGNATURES) and len(image) == 8 and not image & mine
    assert {"nm_bn2d_fwd", "nm_bn2d_bwd"} <= image
    header = open(os.path.join(ROOT, "include", "nmhip_bnsync.h")).read()
    assert "cnn_encoder.py:107" in header and "NM_BN2D_PART_DOUBLES(C) (2 * (C) + 1)" in header


def test_bnsync_entry_points_refuse_before_any_launch(lib):
    """Host buffers and a null stream: a call that got as far as a launch would fault or fail differently."""
    buf = (ctypes.c_float * 65536)()
    other = (ctypes.c_float * 65536)()
    third = (ctypes.c_float * 65536)()
    doubles = (ctypes.c_double * 4096)()

    def check(fn, cases):
        for kwargs, text in cases:
            assert fn(**kwargs) < 0 and lib.nm_last_error() == text, (kwargs, lib.nm_last_error())

    def part(x=buf, ldx=8, rows=30, c=8, out=doubles):
        return lib.nm_bn2d_part_stats(None, x, ldx, rows, c, out)
    check(part, (
        (dict(rows=0), b"nm_bn2d_part_stats: bad sizes rows 0, C 8"), (dict(c=0), b"nm_bn2d_part_stats: bad sizes rows 30, C 0"),
        (dict(rows=1 << 30, c=4), b"nm_bn2d_part_stats: rows * C = 4294967296 elements beyond 2^31 - 1"),
        (dict(x=None), b"nm_bn2d_part_stats: null pointer"), (dict(out=None), b"nm_bn2d_part_stats: null pointer"),
        (dict(ldx=7), b"nm_bn2d_part_stats: ldx 7 below C 8")))

    def merge(parts=doubles, world=3, c=8, mom=0.99, mm=None, mv=None, bm=buf, bv=other, total=ctypes.byref(doubles, 8 * 2048)):
        return lib.nm_bn2d_merge(None, parts, world, c, mom, mm, mv, bm, bv, total)
    check(merge, (
        (dict(world=0), b"nm_bn2d_merge: bad sizes world 0, C 8"), (dict(c=0), b"nm_bn2d_merge: bad sizes world 3, C 0"),
        (dict(c=1 << 31), b"nm_bn2d_merge: world 3 or C 2147483648 beyond 2^31 - 1"),
        (dict(parts=None), b"nm_bn2d_merge: null pointer"), (dict(bm=None), b"nm_bn2d_merge: null pointer"),
        (dict(bv=None), b"nm_bn2d_merge: null pointer"), (dict(total=None), b"nm_bn2d_merge: null pointer"),
        (dict(mm=third), b"nm_bn2d_merge: moving_mean and moving_var come together or not at all"),
        (dict(mv=third), b"nm_bn2d_merge: moving_mean and moving_var come together or not at all"),
        (dict(mom=1.5), b"nm_bn2d_merge: momentum 1.5 outside [0, 1]"),
        (dict(mom=-0.5), b"nm_bn2d_merge: momentum -0.5 outside [0, 1]")))

    def sums(x=buf, ldx=8, y=third, ldy=8, dy=other, lddy=8, rows=30, c=8, mean=third, var=third, eps=1e-3, relu=1,
             out=ctypes.byref(third, 4 * 4096), dg=None, db=None, acc=0):
        return lib.nm_bn2d_bwd_sums(None, x, ldx, y, ldy, dy, lddy, rows, c, mean, var, eps, relu, out, dg, db, acc)
    check(sums, (
        (dict(rows=0), b"nm_bn2d_bwd_sums: bad sizes rows 0, C 8"), (dict(c=-1), b"nm_bn2d_bwd_sums: bad sizes rows 30, C -1"),
        (dict(x=None), b"nm_bn2d_bwd_sums: null pointer"), (dict(dy=None), b"nm_bn2d_bwd_sums: null pointer"),
        (dict(mean=None), b"nm_bn2d_bwd_sums: null pointer"), (dict(var=None), b"nm_bn2d_bwd_sums: null pointer"),
        (dict(out=None), b"nm_bn2d_bwd_sums: null pointer"),
        (dict(y=None), b"nm_bn2d_bwd_sums: the ReLU gate needs the saved output y"),
        (dict(ldx=7), b"nm_bn2d_bwd_sums: ldx 7 below C 8"), (dict(ldy=7), b"nm_bn2d_bwd_sums: ldy 7 below C 8"),
        (dict(lddy=7), b"nm_bn2d_bwd_sums: lddy 7 below C 8"),
        (dict(eps=0.0), b"nm_bn2d_bwd_sums: eps 0 must be positive")))

    def bdx(x=buf, ldx=8, y=third, ldy=8, dy=other, lddy=8, rows=30, c=8, gamma=third, mean=third, var=third, eps=1e-3,
            relu=1, s=ctypes.byref(third, 4 * 4096), n=75, dx=ctypes.byref(other, 4 * 4096), lddx=8, acc=0):
        return lib.nm_bn2d_bwd_dx(None, x, ldx, y, ldy, dy, lddy, rows, c, gamma, mean, var, eps, relu, s, n, dx, lddx, acc)
    check(bdx, (
        (dict(rows=0), b"nm_bn2d_bwd_dx: bad sizes rows 0, C 8"),
        (dict(x=None), b"nm_bn2d_bwd_dx: null pointer"), (dict(dy=None), b"nm_bn2d_bwd_dx: null pointer"),
        (dict(gamma=None), b"nm_bn2d_bwd_dx: null pointer"), (dict(mean=None), b"nm_bn2d_bwd_dx: null pointer"),
        (dict(var=None), b"nm_bn2d_bwd_dx: null pointer"), (dict(s=None), b"nm_bn2d_bwd_dx: null pointer"),
        (dict(dx=None), b"nm_bn2d_bwd_dx: null pointer"),
        (dict(y=None), b"nm_bn2d_bwd_dx: the ReLU gate needs the saved output y"),
        (dict(ldx=7), b"nm_bn2d_bwd_dx: ldx 7 below C 8"), (dict(ldy=7), b"nm_bn2d_bwd_dx: ldy 7 below C 8"),
        (dict(lddy=7), b"nm_bn2d_bwd_dx: lddy 7 below C 8"), (dict(lddx=7), b"nm_bn2d_bwd_dx: lddx 7 below C 8"),
        (dict(eps=-1.0), b"nm_bn2d_bwd_dx: eps -1 must be positive"),
        (dict(n=29), b"nm_bn2d_bwd_dx: global row count 29 below this rank's 30"),
        (dict(n=0), b"nm_bn2d_bwd_dx: global row count 0 below this rank's 30"),
        (dict(dx=ctypes.byref(other, 4 * 40)), b"nm_bn2d_bwd_dx: dx partially overlapping dy")))


def test_kernels_of_the_bnsync_file_do_not_spill(lib):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_resources
    finally:
        sys.path.pop(0)
    mine = {k: v for k, v in kernel_resources().items() if "bnsync_" in k}
    assert len(mine) == 4, sorted(mine)
    assert all(v["scratch"] == 0 for v in mine.values()), {k: v["scratch"] for k, v in mine.items()}
    src = open(os.path.join(ROOT, "neuralmonkey_amd", "csrc", "nm_bnsync.hip")).read()
    names = re.findall(r"__global__.*?void\s+(\w+)\s*\(", src, flags=re.S)
    assert len(names) == 4 and all(n.startswith("bnsync_") for n in names), names


# ---- the model parts under a DataParallel of two ranks --------------------------------------------------------------------
class _TwoRanks:
    """What the model parts and the trainer ask a DataParallel before anything is exchanged; a collective is an error."""
    world_size, rank, forced = 2, 0, False

    def begin_step(self):
        pass

    def __getattr__(self, name):
        raise AssertionError("DataParallel.{} was reached".format(name))


@pytest.fixture
def two_ranks(monkeypatch):
    from neuralmonkey_amd import distributed
    stub = _TwoRanks()
    monkeypatch.setattr(distributed, "_CURRENT", stub)
    assert distributed.current() is stub
    return stub


class _Stop(Exception):
    pass


def _run_objectives(trainer, sess, batch):
    from neuralmonkey_amd.runtime import RunContext
    fd = {}
    for part in trainer.feedables:
        fd.update(part.feed_dict(batch, train=True))
    fd.update(trainer.feed_dict(batch, train=True))
    trainer._objective_gradients(RunContext(sess, fd))        # pylint: disable=protected-access


def test_ctc_decoder_trains_under_two_ranks_with_the_objectives_weight(tmp_path, two_ranks, monkeypatch):
    from neuralmonkey_amd.decoders import CTCDecoder
    from neuralmonkey_amd.trainers import CostObjective, GenericTrainer
    model, _ = ctc_models.load(tmp_path, "speech", "cpu")
    dec = model.runners[0].decoder
    assert isinstance(dec, CTCDecoder) and CTCDecoder.loss_is_batch_sum is True
    assert dec.train_token_count(None) == 1.0                        # no refusal, and no count over the ranks
    trainer = GenericTrainer([CostObjective(dec, weight=0.375)])
    seen = []

    def spy(ctx, want_grad=False, grad_scale=None):
        seen.append((want_grad, grad_scale.clone()))
        raise _Stop()
    monkeypatch.setattr(dec, "_train_loop", spy)
    with pytest.raises(_Stop):                                       # (scale_by_global_count would have been an error)
        _run_objectives(trainer, model.tf_manager.sessions[0], next(iter(model.train_dataset.batches())))
    (want_grad, scale), = seen
    assert want_grad and scale.dtype == torch.float32 and scale.tolist() == [0.375]
    # ... and the trainer of the experiment, weight None = 1
    seen.clear()
    with pytest.raises(_Stop):
        _run_objectives(model.trainers[0], model.tf_manager.sessions[0], next(iter(model.train_dataset.batches())))
    assert seen[0][1].tolist() == [1.0]


def test_reinforce_objective_is_still_refused_under_two_ranks(two_ranks):
    from neuralmonkey_amd import synthetic
    from neuralmonkey_amd.evaluators.gleu import GLEUEvaluator
    from neuralmonkey_amd.trainers import GenericTrainer
    from neuralmonkey_amd.trainers.rl_trainer import ReinforceObjective
    model = synthetic.build_translation_model(vocab_src=40, vocab_tgt=40, emb=8, rnn=8, max_len=6, beam_size=0,
                                              device="cpu", seed=3)
    dec = model.trainer.objectives[0].decoder
    assert not getattr(dec, "loss_is_batch_sum", False)
    trainer = GenericTrainer([ReinforceObjective(dec, GLEUEvaluator())])
    batch = synthetic.synthetic_dataset(seed=5, batch=4, src_len=6, tgt_len=5, vocab=40, ragged=True)
    with pytest.raises(NotImplementedError, match="ReinforceObjective with 2 data-parallel ranks"):
        _run_objectives(trainer, model.tf_manager.sessions[0], batch)


def test_cnn_encoder_no_longer_refuses_ranks_and_stays_out_of_step_graphs():
    import inspect
    from neuralmonkey_amd.encoders import cnn_encoder
    from neuralmonkey_amd.runtime import reset_registry
    reset_registry()
    source = inspect.getsource(cnn_encoder.CNNEncoder)
    assert "NotImplementedError" not in source
    cnn = cnn_encoder.CNNEncoder(name="cnn", data_id="images", convolutions=[("C", 3, 1, "same", 4), ("R", 3, 6)],
                                 image_height=8, image_width=12, pixel_dim=3, batch_normalize=True)
    assert cnn.graph_safe_training(True) is False and "captured step graph" in cnn.graph_safe_training.__doc__
    assert np.prod(cnn.spatial_shape) == 8 * 12 * 6
