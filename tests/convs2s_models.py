"""The convolutional sequence-to-sequence encoder of the tests as engine objects: test infrastructure.

``build``: the model of a fixture of tests/golden/convs2s (make_convs2s_golden.py) -- an EmbeddedSequence with a maximum
length under encoders.facebook_conv.SentenceEncoder, alone or read by a SequenceAveragePooling with both under a
Classifier."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIX = os.path.join(GOLDEN, "convs2s")
BUNDLE = os.path.join(GOLDEN, "reference_tests_convs2s.tar.gz")
LISTS = os.path.join(GOLDEN, "convs2s_signatures.json")
FORWARD_CASES = ["convs2s_k5", "convs2s_k4_one_layer", "convs2s_k3_truncated", "convs2s_classifier",
                 "fd_gradients_convs2s"]
FD_CASES = ["fd_gradients_convs2s"]
LENGTHS = [4, 7, 3, 6, 1]


def load_fixture(case):
    z = np.load(os.path.join(FIX, case + ".npz"))
    return z, json.loads(str(z["cfg"])), {k[2:]: z[k] for k in z.files if k.startswith("p/")}


def words(n):
    from neuralmonkey_amd.vocabulary import Vocabulary
    return Vocabulary(["w{}".format(i) for i in range(n)])


def build_parts(cfg):
    """(sequence, encoder, pooler or None, classifier or None) of a fixture's configuration; no session."""
    from neuralmonkey_amd import tf_shim
    from neuralmonkey_amd.decoders import Classifier
    from neuralmonkey_amd.encoders import SequenceAveragePooling
    from neuralmonkey_amd.encoders.facebook_conv import SentenceEncoder
    from neuralmonkey_amd.model.sequence import EmbeddedSequence
    from neuralmonkey_amd.runtime import reset_registry
    reset_registry()
    seq = EmbeddedSequence(name="encoder_input", vocabulary=words(cfg["src_vocab"]), data_id="source",
                           embedding_size=cfg["emb"], max_length=cfg["max_length"])
    enc = SentenceEncoder(name="encoder", input_sequence=seq, conv_features=cfg["conv_features"],
                          encoder_layers=cfg["encoder_layers"], kernel_width=cfg["kernel_width"])
    avg = dec = None
    if cfg["head"] == "classifier":
        avg = SequenceAveragePooling(name="encoder_avg", input_sequence=enc)
        act = {"relu": tf_shim.nn.relu, "tanh": tf_shim.tanh}[cfg["activation"]]
        dec = Classifier(name="classifier", encoders=[enc, avg], vocabulary=words(cfg["cls_vocab"]), data_id="target",
                         layers=cfg["layers"], activation_fn=act, dropout_keep_prob=1.0)
    return seq, enc, avg, dec


def build(dev, cfg):
    from neuralmonkey_amd.tf_manager import TensorFlowManager
    from neuralmonkey_amd.trainers import CrossEntropyTrainer
    seq, enc, avg, dec = build_parts(cfg)
    feedables = [seq, enc]
    m = dict(seq=seq, enc=enc, avg=avg, dec=dec, trainer=None)
    if dec is not None:
        m["trainer"] = CrossEntropyTrainer(decoders=[dec], l2_weight=0.0, clip_norm=None)
        feedables += [avg, dec]
    tfm = TensorFlowManager(num_sessions=1, num_threads=1, device=str(dev), seed=1)
    tfm.initialize_sessions()
    m.update(tfm=tfm, feedables=feedables, store=tfm.sessions[0].store)
    return m


def dataset_of(z, cfg):
    """The fixture's strings: the source sentences as they were before ``max_length`` cut them, and per sentence the
    target's first token."""
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    src = [str(s).split(" ") for s in z["in/src_sentences"]]
    series = {"source": src}
    if cfg["head"] == "classifier":
        series["target"] = [[str(t)] for t in z["in/tgt_tokens"]]
    return Dataset("fixture", series, BatchingScheme(batch_size=len(src)))


def loaded(dev, case):
    from .test_reference_exec_gpu import load_variables
    z, cfg, params = load_fixture(case)
    m = build(dev, cfg)
    assert load_variables(m["store"], params) == []              # the same variables under the same names, both ways
    ds = dataset_of(z, cfg)
    fd = {}
    for part in m["feedables"]:
        fd.update(part.feed_dict(ds, train=False))
    return z, cfg, params, m, ds, fd
