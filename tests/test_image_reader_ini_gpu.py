"""The reference's tests/str.ini on the MI355X with NO edit: its ``[image_reader]`` section names
``readers.image_reader.image_reader``, which now exists.  The configuration, vocabulary and lists come from the committed
tests/golden/str_tests.tar.gz; under every listed ``.jpg`` name the test writes the decoded pixels of one of the
fixture's group-a sources as PGM / PPM bytes (the reader sniffs content, as Pillow does), so the pixels are the same on
every machine and no Pillow is needed.  The datasets' ``images`` series is then checked against the arrays the
reference's reader produced from those pixels, the model trains and decodes, and the same arrays fed through the
``numpy_reader`` rewrite of the older tests give the CNNEncoder identical inputs.  One more test reads the reference's
real JPEGs through Pillow and compares with the same pipeline called on Pillow directly (JPEG decoders differ between
libjpeg builds, so recorded pixels would not do)."""
import os
import tarfile

import numpy as np
import pytest

from . import cnn2d_models as M
from . import image_reader_ref as ref
from .test_cnn2d_host import with_numpy_images
from .test_reference_inis import load_verbatim

pytestmark = pytest.mark.gpu

F_BOUND = 2.0 ** -15            # mode F against Pillow: see tests/test_image_reader_kernels_gpu.py


def listed(root, split):
    with open(os.path.join(root, "tests", "data", "str", split + "_files.txt")) as handle:
        return [line.rstrip() for line in handle if line.strip()]


@pytest.fixture(scope="module")
def str_tree(tmp_path_factory):
    """-> (root, name -> fixture case): the archive extracted, a PNM file under every listed name."""
    root = str(tmp_path_factory.mktemp("str_verbatim"))
    with tarfile.open(M.BUNDLE) as tar:
        tar.extractall(root)
    cases = ref.cases_of(prefix="a_")
    assert len(cases) == 10
    assigned = {}
    for split in ("val", "train"):
        for j, name in enumerate(listed(root, split)):
            assigned[name] = cases[j % len(cases)]
            with open(os.path.join(root, "tests", "data", "str", name), "wb") as handle:
                handle.write(ref.pnm_bytes(ref.source_of(assigned[name])))
    assert len(assigned) == 40
    return root, assigned


def test_str_ini_loads_verbatim_trains_and_decodes(dev, str_tree):
    """Fails on a tree without the feature with SymbolNotShipped."""
    from neuralmonkey_amd.encoders.cnn_encoder import CNNEncoder
    root, assigned = str_tree
    with open(os.path.join(root, "tests", "str.ini")) as handle:
        assert "class=readers.image_reader.image_reader" in handle.read()
    model = load_verbatim(root, "str", device=str(dev), seed=1234)
    val_names = listed(root, "val")
    images = list(model.val_dataset.get_series("images"))
    assert len(images) == len(val_names) == len(model.val_dataset) == 10
    assert {assigned[n]["name"] for n in val_names} == {c["name"] for c in ref.cases_of(prefix="a_")}   # every a case
    for name, image in zip(val_names, images):
        want = ref.want_of(assigned[name])
        assert image.dtype == np.float32 and image.shape == (32, 256, 1)
        assert np.abs(image - want).max() <= F_BOUND, (name, assigned[name]["name"])
    tfm = model.tf_manager
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    batches = []
    for batch in model.train_dataset.batches():                    # a lazy dataset (buffer_size): the reader streams
        batches.append(batch)
        if len(batches) == 4:
            break
    assert [len(b) for b in batches] == [4, 4, 4, 4]
    cnn = next(p for p in feedables if isinstance(p, CNNEncoder))
    fed = cnn.feed_dict(batches[0], train=True)[cnn.image_input]
    assert fed.dtype == np.float32 and fed.shape == (4, 32, 256, 1) and 0.5 < fed.max() <= 1.0
    losses = []
    for batch in batches:
        res = tfm.execute(batch, feedables, model.trainers, train=True)
        assert res[0].losses and all(np.isfinite(v) for v in res[0].losses.values()), res[0].losses
        losses.append(float(sum(res[0].losses.values())))
    assert tfm.sessions[0].global_step == 4 and np.isfinite(losses).all()
    val = next(iter(model.val_dataset.batches()))
    out = tfm.execute(val, feedables, model.runners, compute_losses=True)[0]
    decoded = out.outputs["target_chars"] if isinstance(out.outputs, dict) else out.outputs
    assert len(decoded) == len(val) == 4 and all(np.isfinite(v) for v in out.losses.values())
    bare = list(model.test_datasets[1].get_series("images"))       # [val_data_no_target]: the same files again
    assert len(bare) == 10 and all(a.tobytes() == b.tobytes() for a, b in zip(bare, images))


def test_numpy_reader_rewrite_feeds_the_cnn_identical_arrays(dev, str_tree):
    from neuralmonkey_amd.encoders.cnn_encoder import CNNEncoder
    root, _ = str_tree
    model = load_verbatim(root, "str", device=str(dev), seed=1234)
    images = list(model.val_dataset.get_series("images"))
    ini = with_numpy_images(root)                                  # the older tests' rewrite, with synthetic images ...
    for name, image in zip(listed(root, "val"), images):           # ... replaced by this reader's arrays
        np.savez(os.path.join(root, "tests", "data", "str_numpy", name + ".npz"), image)
    rewritten = load_verbatim(root, ini, device=str(dev), seed=1234)

    def fed(m):
        cnn = next(p for p in set.union(*[r.feedables for r in m.runners]) if isinstance(p, CNNEncoder))
        batch = next(iter(m.val_dataset.batches()))
        return cnn.feed_dict(batch, train=False)[cnn.image_input]
    mine, theirs = fed(model), fed(rewritten)
    assert mine.dtype == theirs.dtype == np.float32 and mine.shape == theirs.shape == (4, 32, 256, 1)
    assert mine.tobytes() == theirs.tobytes()


def test_real_jpegs_through_pillow_match_pillows_own_resize(dev, tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    from neuralmonkey_amd.readers.image_reader import image_reader
    with tarfile.open(ref.ARCHIVE) as tar:
        names = sorted(m.name for m in tar.getmembers())
        tar.extractall(str(tmp_path))
    prefix = os.path.join(str(tmp_path), "tests", "data", "str")
    listing = os.path.join(str(tmp_path), "files.txt")
    with open(listing, "w") as handle:
        handle.write("\n".join(os.path.basename(n) for n in names) + "\n")
    reader = image_reader(pad_w=256, pad_h=32, channels=1, prefix=prefix, rescale_w=True, rescale_h=True, mode="F")
    got = list(reader([listing]))
    assert len(got) == 40
    differing = 0
    for name, image in zip(names, got):
        want = np.array(Image.open(os.path.join(str(tmp_path), name)).convert("F").resize((256, 32), Image.BILINEAR))
        differing += int((image[:, :, 0] != want).sum())
        assert np.abs(image[:, :, 0] - want).max() <= F_BOUND, name
    print("imgread: 40 JPEGs against Pillow's own resize, {} of {} elements differ".format(differing, 40 * 256 * 32))
