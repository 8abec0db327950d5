"""Generate ``tests/golden/mbr/pairwise.npz``: what the REFERENCE'S OWN ``sentence_bleu`` / ``sentence_gleu`` return on
the tiled sample pairs of the case table of tests/mbr_ref.py -- the utilities of minimum Bayes risk decoding.

Runs only where the reference tree is (nothing at test time needs it).  Like ``make_self_critical_golden.py`` it imports
``make_reference_exec_golden.py`` for the TensorFlow stand-in under which
``neuralmonkey.trainers.self_critical_objective`` imports UNMODIFIED, and calls the two functions on int64 arrays, as
``tf.argmax`` hands them over.  ``sentence_gleu`` asserts where a pair has no n-gram at all on one side; those pairs are
marked in ``gleu_defined`` and hold 0.

    python tests/golden/make_mbr_golden.py

Per case ``<name>``: ``<name>/tok`` [T, B, n] int32, ``<name>/bleu``, ``<name>/gleu`` [B, n, n] float32 ([b, i, j]:
hypothesis sample i, reference sample j) and ``<name>/gleu_defined`` [B, n, n] bool.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_exec_golden as G  # noqa: E402,F401  pylint: disable=wrong-import-position,unused-import

sys.path.insert(0, G.REPO)
from tests import mbr_ref as M  # noqa: E402  pylint: disable=wrong-import-position

OUT = os.path.join(HERE, "mbr", "pairwise.npz")


def main():
    from neuralmonkey.trainers import self_critical_objective as R
    out = {}
    for name, tok in M.cases().items():
        steps, bsz, n = tok.shape
        refs, hyps = M.tile(tok.astype(np.int64))
        out[name + "/tok"] = tok
        out[name + "/bleu"] = R.sentence_bleu(refs, hyps).reshape(bsz, n, n)
        ok = np.ones(refs.shape[1], bool)
        gleu = np.zeros(refs.shape[1], np.float32)
        for m in range(refs.shape[1]):                # (the reference asserts where a sentence has no n-gram at all)
            try:
                with np.errstate(all="ignore"):
                    gleu[m] = R.sentence_gleu(refs[:, m:m + 1], hyps[:, m:m + 1])[0]
            except AssertionError:
                ok[m] = False
        out[name + "/gleu"], out[name + "/gleu_defined"] = gleu.reshape(bsz, n, n), ok.reshape(bsz, n, n)
        print("{:20s} {:6d} pairs, {:4d} without a GLEU".format(name, refs.shape[1], int((~ok).sum())))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
