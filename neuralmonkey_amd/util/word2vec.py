"""Pre-trained embeddings in the word2vec text format (mirror of neuralmonkey/util/word2vec.py).

A file is one header line ``<count> <width>`` and one line ``<word> <width numbers>`` per word.  ``Word2Vec`` makes a
vocabulary and a float64 matrix of it whose row i is the vector of the vocabulary's word i: the four special tokens first
(zero rows unless the file gives them; ``<unk>`` at 3, where the vocabulary looks unknown words up), then the file's
other words in file order.  A configuration hands the vocabulary to a part (``vocabulary=<word2vec.vocabulary>``) and
the matrix to its embedding variable (``initializers=[("word_embeddings", <w2v_init>)]``).

Host code only: the matrix reaches the device with every other initial value, when the variable store is laid out."""
from typing import Callable, List

import numpy as np

from ..checking import check_argument_types
from ..vocabulary import SPECIAL_TOKENS, Vocabulary


class Word2Vec:

    def __init__(self,
                 path: str,
                 encoding: str = "utf-8") -> None:
        """``path``: the word2vec text file; ``encoding``: its encoding."""
        check_argument_types()
        words: List[str] = []
        vectors: List[np.ndarray] = []
        with open(path, encoding=encoding) as f_data:
            header = next(f_data)
            emb_size = int(header.split()[1])
            for _ in SPECIAL_TOKENS:
                vectors.append(np.zeros(emb_size))
            for line in f_data:
                fields = line.split()
                word = fields[0]
                vector = np.fromiter((float(x) for x in fields[1:]), dtype=np.float64)
                assert vector.shape[0] == emb_size
                if word in SPECIAL_TOKENS:
                    vectors[SPECIAL_TOKENS.index(word)] = vector
                else:
                    words.append(word)
                    vectors.append(vector)
        self.vocab = Vocabulary(words)
        self.embedding_matrix = np.stack(vectors)

    @property
    def vocabulary(self) -> Vocabulary:
        """The vocabulary of the file's words."""
        return self.vocab

    @property
    def embeddings(self) -> np.ndarray:
        """The [len(vocabulary), width] float64 embedding matrix."""
        return self.embedding_matrix


def get_word2vec_initializer(w2v: Word2Vec) -> Callable:
    """An initializer that sets a variable to the word2vec matrix.  The reference's is ``init(shape, **kwargs)``
    (TensorFlow's calling convention); initializers of this package are ``init(rng, shape)`` (variables.py), and the
    variable store rounds what they return to float32 -- once, from the file's float64 values."""
    check_argument_types()

    def init(rng, shape) -> np.ndarray:                                       # pylint: disable=unused-argument
        if list(shape) != list(w2v.embeddings.shape):
            raise ValueError(
                "Shapes of model and word2vec embeddings do not match. "
                "Word2Vec shape: {}, Should have been: {}"
                .format(w2v.embeddings.shape, list(shape)))
        return w2v.embeddings

    return init


def word2vec_vocabulary(w2v: Word2Vec) -> Vocabulary:
    """The vocabulary of a word2vec object (for configurations)."""
    check_argument_types()
    return w2v.vocabulary
