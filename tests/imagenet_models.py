"""What the ImageNet tests share: the reference's tests/captioning.ini with its data from the committed archives, the two
rewrites of it the tests need, and the narrow width table.

tests/captioning.ini AS IT IS cannot be built by the reference either: its decoder has ``rnn_size=8`` and
``embedding_size=9`` and no output projection, which decoders/decoder.py:337-342 of the reference refuses with a
ValueError ("The dimension (8) of the output projection must be same as the dimension of the input embedding (9)"); the
configuration is commented out in the reference's tests/tests_run.sh.  This engine mirrors that refusal
(decoders/decoder.py), as tests/test_alignment_host.py pins for tests/alignment.ini.  So the verbatim file is pinned to
that error -- which its ``[imagenet]`` section has to be built to reach -- and everything else is asserted on the file
with that ONE value changed (``rnn_size=9``)."""
import os
import re
import tarfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
TEXT_BUNDLE = os.path.join(GOLDEN, "reference_tests.tar.gz")          # lists, captions, decoder_vocab.tsv
# the 13 JPEGs of tests/data/flickr30k and tests/captioning.ini itself, in two archives below the size limit of a file
IMAGE_BUNDLES = [os.path.join(GOLDEN, "reference_tests_flickr_images_{}.tar.gz".format(part)) for part in "ab"]
REFUSAL = "The dimension (8) of the output projection must be same as the dimension of the input embedding (9)"
NARROW = {"conv": (4, 8, 16, 32, 32), "fc": (64, 64), "classes": 10}


def extract(root):
    for bundle in [TEXT_BUNDLE] + IMAGE_BUNDLES:
        with tarfile.open(bundle) as tar:
            tar.extractall(root)
    return str(root)


def sections(text):
    parts = re.split(r"(?m)^(?=\[[a-z_]+\]$)", text)
    return {re.match(r"\[([a-z_]+)\]", p).group(1): p for p in parts if p.startswith("[")}


def with_rnn_size(root, source="captioning", name="captioning_rnn9"):
    """The file with ``rnn_size=8`` -> ``rnn_size=9`` and nothing else; -> the new INI's name."""
    text = open(os.path.join(root, "tests", source + ".ini")).read()
    edited, n = re.subn(r"(?m)^rnn_size=8$", "rnn_size=9", text)
    assert n == 1
    before, after = sections(text), sections(edited)
    assert [k for k in before if before[k] != after[k]] == ["decoder"] and set(before) == set(after)
    with open(os.path.join(root, "tests", name + ".ini"), "w") as handle:
        handle.write(edited)
    return name


def with_numpy_images(root, source, name, seed=11):
    """``source`` with its [image_reader] section alone replaced by the NumPy reader over synthetic 224 x 224 x 3 arrays
    written here, one per name of the reference's two lists (for machines without a GPU: the image reader resizes on
    the device); -> the new INI's name."""
    rng = np.random.default_rng(seed)
    data = os.path.join(root, "tests", "data", "flickr30k")
    images = os.path.join(root, "tests", "data", "flickr30k_numpy")
    os.makedirs(images, exist_ok=True)
    for split in ("train", "val"):
        for line in open(os.path.join(data, split + "_images.txt")).read().split("\n"):
            if line:
                np.savez(os.path.join(images, line + ".npz"), rng.uniform(-124.0, 152.0, (224, 224, 3)).astype(np.float32))
    text = open(os.path.join(root, "tests", source + ".ini")).read()
    edited, n = re.subn(r"\[image_reader\]\n(?:[^\[\n][^\n]*\n)+",
                        '[image_reader]\nclass=readers.numpy_reader.from_file_list\nprefix="{}"\n'
                        'shape=[224, 224, 3]\nsuffix=".npz"\n'.format(images), text)
    assert n == 1
    before, after = sections(text), sections(edited)
    assert [k for k in before if before[k] != after[k]] == ["image_reader"] and set(before) == set(after)
    with open(os.path.join(root, "tests", name + ".ini"), "w") as handle:
        handle.write(edited)
    return name


def narrow(monkeypatch):
    """The width tables of both networks shrunk: conv widths 4, 8, 16, 32, 32, fc width 64, 10 classes."""
    from neuralmonkey_amd.encoders import imagenet_encoder as E
    monkeypatch.setattr(E, "NETWORK_WIDTHS", {"vgg_16": dict(NARROW), "vgg_19": dict(NARROW)})
    return NARROW
