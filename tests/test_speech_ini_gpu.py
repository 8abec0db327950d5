"""The reference's two speech configurations on the MI355X, from the committed archive
tests/golden/reference_tests_audio.tar.gz: tests/audio-classifier.ini (DTMF tones -> MFCC + deltas -> RecurrentEncoder ->
Classifier) and tests/ctc.ini (yes/no recordings -> MFCC + two delta orders -> stacked RecurrentEncoder -> CTCDecoder),
both files byte for byte.  The archive carries six of the fifteen yes/no recordings (all of them would pass the limit
for a committed file), so the two list files and the two transcripts of tests/data/yesno are cut to the four and two
lines whose recordings are there; the configuration itself is not touched.

The datasets are eager, so loading a configuration reads every recording and runs the feature kernels: the feature
series are checked against tests/speech_ref.py, then a few optimizer steps must lower the loss and the file's runner
must decode a validation batch."""
import os
import tarfile

import numpy as np
import pytest

from . import speech_ref
from .test_speech_host import BUNDLE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def audio_tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("reference_tests_audio_gpu")
    with tarfile.open(BUNDLE) as tar:
        tar.extractall(root)
    yesno = os.path.join(str(root), "tests", "data", "yesno")
    for name, keep in (("train.wavlist", 4), ("train.txt", 4), ("test.wavlist", 2), ("test.txt", 2)):
        with open(os.path.join(yesno, name)) as handle:
            lines = handle.readlines()[:keep]
        with open(os.path.join(yesno, name), "w") as handle:
            handle.writelines(lines)
    return str(root)


def load(root, name, dev, **kw):
    from .test_reference_inis import load_verbatim
    return load_verbatim(root, name, device=str(dev), **kw)


def check_features(dataset, series, width, order):
    """Frame counts and widths of a feature series against the restatement; the values against it on the first and the
    last item (the last one's rows lie inside the ragged batch that ``dataset.load`` hands to ``many``)."""
    audios, feats = list(dataset.get_series("audio")), list(dataset.get_series(series))
    assert len(audios) == len(feats) == len(dataset) > 0
    for audio, feat in zip(audios, feats):
        frame_len, frame_step, _ = speech_ref.framing(audio.rate)
        assert feat.dtype == np.float32 and feat.shape == (speech_ref.num_frames(len(audio.data), frame_len, frame_step),
                                                           width)
        assert np.isfinite(feat).all()
    for item in (0, len(audios) - 1):
        ref = speech_ref.features(audios[item].data, audios[item].rate, "mfcc", delta_order=order)
        again = speech_ref.features(audios[item].data, audios[item].rate, "mfcc", delta_order=order, dtype=np.float32)
        assert np.abs(feats[item] - ref).max() <= max(8 * np.abs(again - ref).max(), 1e-5), item


def train(model, steps):
    """``steps`` optimizer steps on the first training batch (with the file's dropout); returns the feedables and the
    batch's loss as the file's runner reports it -- in inference mode, so without dropout noise -- before and after."""
    tfm = model.tf_manager
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    batch = next(iter(model.train_dataset.batches()))

    def runner_loss():
        out = tfm.execute(batch, feedables, model.runners, compute_losses=True)[0]
        return float(next(value for key, value in sorted(out.losses.items()) if "train" in key))
    before = runner_loss()
    costs = [float(tfm.execute(batch, feedables, model.trainers, train=True)[0].losses["decoder - cost"])
             for _ in range(steps)]
    after = runner_loss()
    assert tfm.sessions[0].global_step == steps and np.isfinite(costs).all() and np.isfinite([before, after]).all()
    print("speech ini: the batch's loss before {:.4f} and after {:.4f} {} steps".format(before, after, steps))
    return feedables, before, after


def test_audio_classifier_ini_loads_trains_and_decodes(dev, audio_tree):
    """Fails on a tree without the feature with SymbolNotShipped."""
    from neuralmonkey_amd.config.builder import OutOfScope
    from neuralmonkey_amd.decoders.classifier import Classifier
    from neuralmonkey_amd.runners import GreedyRunner
    model = load(audio_tree, "audio-classifier", dev)
    assert isinstance(model.runners[0], GreedyRunner) and isinstance(model.runners[0].decoder, Classifier)
    assert isinstance(model.evaluation[0][-1], OutOfScope)               # evaluators.Accuracy stays a placeholder
    assert len(model.train_dataset) == 9 and len(model.val_dataset) == 3 and model.batch_size == 2
    assert model.train_dataset.series == ["audio", "features", "target"]
    check_features(model.train_dataset, "features", 26, 1)
    check_features(model.val_dataset, "features", 26, 1)
    assert [f.shape[0] for f in model.train_dataset.get_series("features")][:1] == [42]
    model = load(audio_tree, "audio-classifier", dev, changes=["tf_manager.seed=1234"])
    feedables, before, after = train(model, 40)
    assert after < before
    val = next(iter(model.val_dataset.batches()))
    out = model.tf_manager.execute(val, feedables, model.runners, compute_losses=True)[0]
    labels = out.outputs["target"]
    words = set(model.runners[0].decoder.vocabulary.index_to_word)
    assert len(labels) == len(val) == 2 and all(len(s) <= 1 and set(s) <= words for s in labels)


def test_ctc_ini_loads_trains_and_decodes(dev, audio_tree):
    from neuralmonkey_amd.config.builder import OutOfScope
    from neuralmonkey_amd.decoders.ctc_decoder import CTCDecoder
    from neuralmonkey_amd.runners import PlainRunner
    model = load(audio_tree, "ctc", dev)
    assert isinstance(model.runners[0], PlainRunner) and isinstance(model.runners[0].decoder, CTCDecoder)
    assert isinstance(model.evaluation[0][-1], OutOfScope)               # evaluators.WER stays a placeholder
    assert len(model.train_dataset) == 4 and len(model.val_dataset) == 2 and model.batch_size == 4
    check_features(model.train_dataset, "source", 39, 2)
    check_features(model.val_dataset, "source", 39, 2)
    assert [f.shape[0] for f in model.val_dataset.get_series("source")][:1] == [629]
    model = load(audio_tree, "ctc", dev, changes=["tf_manager.seed=1234"])
    feedables, before, after = train(model, 5)
    assert after < before
    val = next(iter(model.val_dataset.batches()))
    out = model.tf_manager.execute(val, feedables, model.runners, compute_losses=True)[0]
    sentences = out.outputs["target"]
    frames = [f.shape[0] for f in val.get_series("source")]
    words = set(model.runners[0].decoder.vocabulary.index_to_word)
    assert len(sentences) == 2 and all(len(s) <= n and set(s) <= words for s, n in zip(sentences, frames))
