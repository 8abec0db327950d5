"""A tagging experiment and a masked-language-model experiment of the tests as INI text plus their synthetic data
files: test infrastructure.

``tagger``: EmbeddedSequence -> RecurrentEncoder (bidirectional GRU) -> SequenceLabeler (hidden layer, tanh) under
CrossEntropyTrainer, decoded by LabelRunner -- the class paths of the reference's tests/labeler.ini.  ``mlm``:
EmbeddedSequence -> TransformerEncoder -> EmbeddingsLabeler over the same sequence's table, LabelRunner + XentRunner
-- those of tests/bert.ini.  The tag of a word is a function of the word, so a few steps lower the cost."""
import numpy as np

WORDS = ["w{}".format(i) for i in range(12)]
TAGS = ["N", "V", "A", "D"]

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
runners=[{runners}]
evaluation=[("tags", evaluators.Accuracy)]
logging_period=1
validation_period=5
random_seed=123485

[tf_manager]
class=tf_manager.TensorFlowManager
num_threads=4
num_sessions=1
seed=1234

[train_data]
class=dataset.load
series=["source", "tags"]
data=["{root}/source.txt", "{root}/tags.txt"]

[source_vocabulary]
class=vocabulary.from_wordlist
path="{root}/words.vocab"
contains_header=False
contains_frequencies=False

[tags_vocabulary]
class=vocabulary.from_wordlist
path="{root}/tags.vocab"
contains_header=False
contains_frequencies=False

[encoder_input]
class=model.sequence.EmbeddedSequence
name="encoder_input"
embedding_size=8
data_id="source"
vocabulary=<source_vocabulary>

[trainer]
class=trainers.cross_entropy_trainer.CrossEntropyTrainer
decoders=[<decoder>]
l2_weight=1.0e-8
optimizer=<optimizer>

[optimizer]
class=tf.train.AdamOptimizer
learning_rate={lr}

[runner]
class={runner_class}
decoder=<decoder>
output_series="tags"

[runner_xent]
class=runners.XentRunner
decoder=<decoder>
output_series="xent"
"""

TAGGER = """
[encoder]
class=encoders.RecurrentEncoder
name="encoder"
input_sequence=<encoder_input>
rnn_layers=[(6, "bidirectional", "GRU")]
dropout_keep_prob={keep}

[decoder]
class=decoders.sequence_labeler.SequenceLabeler
name="tagger"
encoders=[<encoder>]
data_id="tags"
vocabulary=<tags_vocabulary>
hidden_dim=10
activation=tf.tanh
dropout_keep_prob={keep}
{decoder_extra}
"""

MLM = """
[encoder]
class=encoders.transformer.TransformerEncoder
name="encoder"
input_sequence=<encoder_input>
ff_hidden_size=12
depth=2
n_heads=2
dropout_keep_prob={keep}

[decoder]
class=decoders.sequence_labeler.EmbeddingsLabeler
name="tagger"
encoders=[<encoder>]
embedded_sequence=<encoder_input>
data_id="tags"
dropout_keep_prob={keep}
{decoder_extra}
"""


def write_data(root, kind, n=12, seed=0):
    """Sentences of 1..9 words (the first has one word).  ``tagger``: the tag of word i is TAGS[i % 4].  ``mlm``: the
    target repeats the word at about half of the positions and is <pad> at the others."""
    rng = np.random.default_rng(seed)
    (root / "words.vocab").write_text("".join(w + "\n" for w in WORDS))
    (root / "tags.vocab").write_text("".join(t + "\n" for t in TAGS))
    src = [[str(w) for w in rng.choice(WORDS, size=1 if i == 0 else int(rng.integers(2, 10)))] for i in range(n)]
    if kind == "tagger":
        tags = [[TAGS[int(w[1:]) % len(TAGS)] for w in s] for s in src]
    else:
        tags = [[w if rng.random() < 0.5 or j == 0 else "<pad>" for j, w in enumerate(s)] for s in src]
    (root / "source.txt").write_text("".join(" ".join(s) + "\n" for s in src))
    (root / "tags.txt").write_text("".join(" ".join(t) + "\n" for t in tags))
    return src, tags


def ini_text(root, kind, batch=12, keep=1.0, lr=0.02, decoder_extra="", runner_class="runners.LabelRunner",
             runners="<runner>"):
    body = TAGGER if kind == "tagger" else MLM
    return (HEAD.format(name="label " + kind, root=root, batch=batch, lr=lr, runner_class=runner_class, runners=runners)
            + body.format(keep=keep, decoder_extra=decoder_extra))


def load(root, kind, device, **kw):
    from neuralmonkey_amd.config.configuration import load_experiment
    data = write_data(root, kind)
    path = root / "label_{}.ini".format(kind)
    path.write_text(ini_text(root, kind, **kw))
    return load_experiment(str(path), device=str(device), seed=1234), data
