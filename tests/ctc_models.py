"""The two CTC experiments of the tests as INI text plus their synthetic data files: test infrastructure.

``speech``: TemporalFiller(39) -> RecurrentEncoder [(50, bidirectional), (100, forward), (100, backward)] -> CTCDecoder,
the model sections of the reference's tests/ctc.ini; the features come through readers.numpy_reader (the audio reader
and the MFCC preprocessor of that file belong to the control plane).  ``chars``: EmbeddedSequence ->
SentenceCNNEncoder -> CTCDecoder, a character-level encoder under the same head."""
import numpy as np

WORDS = ["yes", "no", "maybe"]

HEAD = """
[main]
name="{name}"
tf_manager=<tf_manager>
output="{root}/out"
overwrite_output_dir=True
batch_size={batch}
epochs=1
train_dataset=<train_data>
val_dataset=<train_data>
trainer=<trainer>
runners=[<runner>]
evaluation=[("target", evaluators.WER)]
logging_period=1
validation_period=5
random_seed=123485

[tf_manager]
class=tf_manager.TensorFlowManager
num_threads=4
num_sessions=1

[decoder_vocabulary]
class=vocabulary.from_wordlist
path="{root}/words.vocab"
contains_header=False
contains_frequencies=False

[decoder]
class=decoders.ctc_decoder.CTCDecoder
encoder=<encoder>
vocabulary=<decoder_vocabulary>
data_id="target"
name="decoder"
{decoder_extra}

[trainer]
class=trainers.cross_entropy_trainer.CrossEntropyTrainer
decoders=[<decoder>]
l2_weight=1.0e-8
optimizer=<optimizer>

[optimizer]
class=tf.train.AdamOptimizer
learning_rate={lr}

[runner]
class=runners.PlainRunner
decoder=<decoder>
output_series="target"
"""

SPEECH = """
[train_data]
class=dataset.load
series=["source", "target"]
data=[("{root}/features.npy", readers.numpy_reader.single_tensor), "{root}/train.txt"]

[input_seq]
class=encoders.numpy_stateful_filler.TemporalFiller
data_id="source"
input_size=39

[encoder]
class=encoders.RecurrentEncoder
name="audio_encoder"
input_sequence=<input_seq>
rnn_layers=[(50,"bidirectional"),(100,"forward"),(100,"backward")]
dropout_keep_prob={keep}
"""

CHARS = """
[train_data]
class=dataset.load
series=["source", "target"]
data=["{root}/chars.txt", "{root}/train.txt"]

[char_vocabulary]
class=vocabulary.from_wordlist
path="{root}/chars.vocab"
contains_header=False
contains_frequencies=False

[input_seq]
class=model.sequence.EmbeddedSequence
name="char_input"
vocabulary=<char_vocabulary>
data_id="source"
embedding_size=12
max_length=24

[encoder]
class=encoders.SentenceCNNEncoder
name="char_encoder"
input_sequence=<input_seq>
segment_size=2
highway_depth=1
rnn_size=16
filters=[(1,8), (3,8)]
dropout_keep_prob={keep}
"""


def write_data(root, kind, n=8, seed=0, frames=21):
    """Targets of 0..4 words (one line each, the first line empty), and per example either [frames, 39] features whose
    mean drifts with the words, or a character line of 6..24 symbols."""
    rng = np.random.default_rng(seed)
    (root / "words.vocab").write_text("".join(w + "\n" for w in WORDS))
    targets = [[]] + [[str(w) for w in rng.choice(WORDS, size=int(rng.integers(1, 5)))] for _ in range(n - 1)]
    targets[1] = ["no", "no", "yes"]                                   # a repeated label
    (root / "train.txt").write_text("".join(" ".join(t) + "\n" for t in targets))
    if kind == "speech":
        feats = rng.standard_normal((n, frames, 39)).astype(np.float32)
        for i, t in enumerate(targets):
            for j, w in enumerate(t):
                feats[i, 4 * j:4 * j + 4, :8] += 1.5 * (WORDS.index(w) + 1)
        np.save(root / "features.npy", feats)
    else:
        chars = list("abcdefgh")
        (root / "chars.vocab").write_text("".join(c + "\n" for c in chars))
        lines = [" ".join(rng.choice(chars, size=int(rng.integers(6, 25)))) for _ in range(n)]
        (root / "chars.txt").write_text("".join(l + "\n" for l in lines))
    return targets


def ini_text(root, kind, batch=8, keep=1.0, lr=0.01, decoder_extra=""):
    body = SPEECH if kind == "speech" else CHARS
    return (HEAD.format(name="ctc " + kind, root=root, batch=batch, lr=lr, decoder_extra=decoder_extra)
            + body.format(root=root, keep=keep))


def load(root, kind, device, **kw):
    from neuralmonkey_amd.config.configuration import load_experiment
    targets = write_data(root, kind)
    path = root / "ctc_{}.ini".format(kind)
    path.write_text(ini_text(root, kind, **kw))
    return load_experiment(str(path), device=str(device), seed=1234), targets
