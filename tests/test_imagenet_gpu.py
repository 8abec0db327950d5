"""The ImageNet encoder on the MI355X: narrow VGG-16 / VGG-19 end to end against tests/imagenet_ref.py, the checkpoint
round trip under slim's names, the reference's tests/captioning.ini from the committed archives (with the one value
changed that the reference itself needs changed: tests/imagenet_models.py), and the encoder as a drop-in for the
SpatialFiller of tests/flat-multiattention.ini.

No bound for a chain of 16 to 19 layers can be derived, so the end-to-end comparison is relative: the same restatement
runs in torch float32 on the CPU as well, and the engine's maximum error against the float64 run, over max |want|, may be
at most 4 times torch-float32's, per endpoint.  Both are fp32 sums in different orders; the factor covers the different
order only.  The test prints both errors; DESIGN.md section 4.20 records them."""
import os
import re

import numpy as np
import pytest
import torch

from . import imagenet_models as M
from . import imagenet_ref as ref
from .test_reference_inis import load_verbatim

pytestmark = pytest.mark.gpu

FACTOR = 4.0


def images_of(seed, count=2):
    rng = np.random.default_rng(seed)
    return rng.uniform(-124.0, 152.0, (count, 224, 224, 3)).astype(np.float32)          # 0 .. 255 minus the VGG means


def build(dev, parts_kw, net):
    """Parts over one session; -> (parts, tfm, store)."""
    from neuralmonkey_amd.encoders.imagenet_encoder import ImageNet
    from neuralmonkey_amd.runtime import reset_registry
    from neuralmonkey_amd.tf_manager import TensorFlowManager
    reset_registry()
    parts = [ImageNet(name="part{}".format(i), data_id="images", network_type=net, slim_models_path="unused", **kw)
             for i, kw in enumerate(parts_kw)]
    tfm = TensorFlowManager(num_sessions=1, num_threads=1, device=str(dev), seed=1)
    tfm.initialize_sessions()
    return parts, tfm, tfm.sessions[0].store


def dataset_of(images):
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    return Dataset("images", {"images": list(images)}, BatchingScheme(batch_size=len(images)))


def run(tfm, parts, fetches, images):
    feed = {}
    ds = dataset_of(images)
    for part in parts:
        feed.update(part.feed_dict(ds, train=False))
    out = tfm.sessions[0].run(fetches, feed)
    return {k: None if v is None else np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def relative_check(label, got, want64, want32):
    scale = float(np.abs(want64).max())
    mine = float(np.abs(got.astype(np.float64) - want64).max()) / scale
    theirs = float(np.abs(want32.astype(np.float64) - want64).max()) / scale
    print("imagenet {}: engine {:.3e}, torch float32 {:.3e} (max error over max |want|)".format(label, mine, theirs))
    assert got.shape == want64.shape and np.isfinite(got).all() and scale > 0
    assert mine <= FACTOR * theirs, (label, mine, theirs)


# ---- narrow networks end to end -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["vgg_16", "vgg_19"])
def test_narrow_network_matches_the_float64_restatement(dev, monkeypatch, net):
    widths = M.narrow(monkeypatch)
    mid, last, pool5, fc7 = (net + s for s in ("/conv3/conv3_2", "/conv5/conv5_3", "/pool5", "/fc7"))
    parts, tfm, store = build(dev, [dict(spatial_layer=last), dict(spatial_layer=pool5, encoded_layer=fc7),
                                    dict(spatial_layer=mid)], net)
    variables = ref.random_variables(net, widths, seed=5, upto=fc7)
    assert sorted(store.names()) == sorted(variables) and store.trainable_names() == []
    store.load_state_dict(variables)
    images = images_of(7)
    want64 = ref.forward(net, variables, images, widths, upto=fc7)
    want32 = ref.forward(net, variables, images, widths, upto=fc7, dtype=torch.float32)
    a, b, c = parts
    got = run(tfm, parts, {"last": a.spatial_states, "mask": a.spatial_mask, "mean": a.output, "pool5": b.spatial_states,
                           "fc7": b.output, "mid": c.spatial_states, "mid_mask": c.spatial_mask}, images)
    assert got["last"].shape == (2, 14, 14, 32) and got["pool5"].shape == (2, 7, 7, 32) and got["mid"].shape == (2, 56, 56, 16)
    assert got["mask"].shape == (2, 14, 14) and (got["mask"] == 1.0).all() and (got["mid_mask"] == 1.0).all()
    assert got["mean"].shape == (2, 32) and got["fc7"].shape == (2, 64)
    relative_check(net + " conv3_2", got["mid"], want64[mid], want32[mid])
    relative_check(net + " conv5_3", got["last"], want64[last], want32[last])
    relative_check(net + " pool5", got["pool5"], want64[pool5], want32[pool5])
    relative_check(net + " output (mean of conv5_3)", got["mean"], want64[last].mean(axis=(1, 2)),
                   want32[last].mean(axis=(1, 2), dtype=np.float32))
    relative_check(net + " output (fc7)", got["fc7"], want64[fc7][:, 0, 0, :], want32[fc7][:, 0, 0, :])
    assert (want64[last] == 0).mean() > 0.1 and (want64[last] > 0).mean() > 0.1          # the ReLUs cut, and not everything


# ---- checkpoints ------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_under_slims_names(dev, monkeypatch, tmp_path):
    from neuralmonkey_amd import tf_bundle
    widths = M.narrow(monkeypatch)
    net, last = "vgg_16", "vgg_16/conv5/conv5_3"
    everything = ref.random_variables(net, widths, seed=9)                     # ... to fc8
    mine = ref.random_variables(net, widths, seed=9, upto=last)
    assert set(mine) < set(everything) and "vgg_16/fc8/weights" in everything and all(
        np.array_equal(mine[k], everything[k]) for k in mine)
    exact, more = str(tmp_path / "exact.ckpt"), str(tmp_path / "whole.ckpt")
    tf_bundle.write_bundle(exact, mine)
    tf_bundle.write_bundle(more, everything)
    images = images_of(3)
    want64 = ref.forward(net, mine, images, widths, upto=last)[last]
    want32 = ref.forward(net, mine, images, widths, upto=last, dtype=torch.float32)[last]
    for path in (exact, more):
        (part,), tfm, store = build(dev, [dict(spatial_layer=last, load_checkpoint=path)], net)
        assert sorted(store.names()) == sorted(mine)
        before = {n: store[n].clone() for n in store.names()}
        part.load(tfm.sessions[0])
        assert all(np.array_equal(store[n].cpu().numpy(), mine[n]) for n in mine)
        assert any(not torch.equal(before[n], store[n]) for n in mine)
        got = run(tfm, [part], {"states": part.spatial_states}, images)["states"]
        relative_check("restored from " + os.path.basename(path), got, want64, want32)
    saved = str(tmp_path / "saved.ckpt")
    part._save_checkpoint = saved                                               # pylint: disable=protected-access
    part.save(tfm.sessions[0])
    back = tf_bundle.read_bundle(saved)
    assert sorted(back) == sorted(mine) and all(n.startswith("vgg_16/") for n in back)
    assert all(back[n].shape == mine[n].shape and np.array_equal(back[n], mine[n]) for n in mine)
    with pytest.raises(KeyError, match="lacks variable 'vgg_16/conv5/conv5_3/"):
        short = str(tmp_path / "short.ckpt")
        tf_bundle.write_bundle(short, {k: v for k, v in mine.items() if "conv5_3" not in k})
        (part,), tfm, _ = build(dev, [dict(spatial_layer=last, load_checkpoint=short)], net)
        part.load(tfm.sessions[0])


# ---- tests/captioning.ini ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def captioning_root(tmp_path_factory):
    return M.extract(tmp_path_factory.mktemp("captioning_gpu"))


def test_captioning_ini_trains_and_decodes_from_the_jpegs(dev, captioning_root):
    """The reference's file with ``rnn_size=9`` (tests/imagenet_models.py), its reader over the reference's 13 JPEGs:
    both training batches of the epoch with dropout, then GreedyRunner on the validation set.  Fails on a tree without the
    feature with SymbolNotShipped."""
    pytest.importorskip("PIL")
    from neuralmonkey_amd.encoders.imagenet_encoder import ImageNet
    with open(os.path.join(captioning_root, "tests", "captioning.ini")) as handle:
        text = handle.read()
    assert "class=encoders.imagenet_encoder.ImageNet" in text and "class=readers.image_reader.imagenet_reader" in text
    model = load_verbatim(captioning_root, M.with_rnn_size(captioning_root), device=str(dev), seed=1234)
    tfm = model.tf_manager
    sess = tfm.sessions[0]
    store = sess.store
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    enc = next(p for p in feedables if isinstance(p, ImageNet))
    frozen = {n: store[n].clone() for n in store.names() if n.startswith("vgg_16/")}
    assert len(frozen) == 26 and sum(v.numel() for v in frozen.values()) == 14714688
    assert not set(frozen) & set(store.trainable_names())
    others = {n: store[n].clone() for n in store.trainable_names()}
    batches = list(model.train_dataset.batches())
    assert [len(b) for b in batches] == [5, 5]
    for batch in batches:
        res = tfm.execute(batch, feedables, model.trainers, train=True)[0]
        assert res.losses and all(np.isfinite(v) for v in res.losses.values()), res.losses
    assert sess.global_step == 2
    for name, before in frozen.items():
        assert torch.equal(store[name], before), name                              # bit-identical after the steps
    assert any(not torch.equal(store[n], before) for n, before in others.items())  # ... while the rest trained
    assert store.adam_m is not None
    for name in frozen:                                                            # no optimizer state ever reached them
        spec = store.specs[name]
        assert not store.adam_m[spec.offset:spec.offset + spec.size].any(), name
    val = next(iter(model.val_dataset.batches()))
    assert len(val) == len(model.val_dataset) == 3
    out = tfm.execute(val, feedables, model.runners, compute_losses=True)[0]
    decoded = out.outputs["target"] if isinstance(out.outputs, dict) else out.outputs
    assert len(decoded) == 3 and all(len(s) <= 10 for s in decoded)
    assert all(np.isfinite(v) for v in out.losses.values())
    feed = enc.feed_dict(val, train=False)
    assert feed[enc.image_input].shape == (3, 224, 224, 3) and feed[enc.image_input].dtype == np.float32
    assert feed[enc.image_input].min() < -100.0 and feed[enc.image_input].max() > 100.0       # the VGG means are off
    got = {k: np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in sess.run(
        {"states": enc.spatial_states, "mask": enc.spatial_mask, "output": enc.output}, feed).items()}
    assert got["states"].shape == (3, 14, 14, 512) and got["mask"].shape == (3, 14, 14)
    assert (got["mask"] == 1.0).all() and np.isfinite(got["states"]).all()
    assert got["output"].shape == (3, 512) and got["states"].min() == 0.0 and got["states"].max() > 0.0


# ---- a drop-in for the SpatialFiller of tests/flat-multiattention.ini -------------------------------------------------------
def test_flat_multiattention_ini_over_the_narrow_network(dev, captioning_root, monkeypatch):
    pytest.importorskip("PIL")
    from neuralmonkey_amd.encoders.imagenet_encoder import ImageNet
    M.narrow(monkeypatch)
    text = open(os.path.join(captioning_root, "tests", "flat-multiattention.ini")).read()
    before = M.sections(text)
    edited, n = re.subn(r"\[numpy_reader\]\n(?:[^\[\n][^\n]*\n)+",
                        '[numpy_reader]\nclass=readers.image_reader.imagenet_reader\nprefix="tests/data/flickr30k"\n'
                        "target_width=224\ntarget_height=224\nvgg_normalization=True\n", text)
    edited, m = re.subn(r"\[imagenet\]\n(?:[^\[\n][^\n]*\n)+",
                        '[imagenet]\nclass=encoders.imagenet_encoder.ImageNet\nname="imagenet"\ndata_id="images"\n'
                        'network_type="vgg_16"\nspatial_layer="vgg_16/conv5/conv5_3"\nslim_models_path="unused"\n', edited)
    assert n == 1 and m == 1 and edited.count("_images.npz.txt") == 2
    edited = edited.replace("_images.npz.txt", "_images.txt")
    after = M.sections(edited)
    assert sorted(k for k in before if before[k] != after[k]) == ["imagenet", "numpy_reader", "train_data", "val_data"]
    with open(os.path.join(captioning_root, "tests", "flat-multiattention-vgg.ini"), "w") as handle:
        handle.write(edited)
    model = load_verbatim(captioning_root, "flat-multiattention-vgg", device=str(dev), seed=1234)
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    enc, = [p for p in feedables if isinstance(p, ImageNet)]
    assert enc.dimension == 32 and len(model.trainers[0].objectives) == 4
    store = model.tf_manager.sessions[0].store
    frozen = {n: store[n].clone() for n in store.names() if n.startswith("vgg_16/")}
    assert len(frozen) == 26
    batch = next(iter(model.train_dataset.batches()))
    res = model.tf_manager.execute(batch, feedables, model.trainers, train=True)[0]
    assert res.losses and all(np.isfinite(v) for v in res.losses.values()), res.losses
    assert all(torch.equal(store[n], v) for n, v in frozen.items())
    outs = model.tf_manager.execute(batch, feedables, model.runners)
    assert len(outs) == len(model.runners) == 5
    for out in outs:
        (_, sents), = out.outputs.items()
        assert len(sents) == len(batch)
