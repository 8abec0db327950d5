"""chrF without a GPU: SentenceChrF on the host against tests/chrf_ref.py and the reference's fixed points, its
constructor's refusals and its character table, the entry points in their header, binding table and wrappers, and the
arguments they refuse (before a launch, so no device is needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

from . import chrf_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (n, beta, ignored_symbols, join_subwords): the variants of the GPU tests
VARIANTS = [(6, 1.0, None, False), (6, 3.0, None, False), (1, 2.0, None, False), (4, 1.0, None, False),
            (6, 1.0, [" "], False), (6, 1.0, None, True)]


@pytest.mark.parametrize("n,beta,ignored,join", VARIANTS)
def test_the_host_rule_is_the_counter_restatement(n, beta, ignored, join):
    from neuralmonkey_amd.trainers.self_critical_objective import SentenceChrF
    vocab, lengths = C.vocabulary(), set()
    chrf = SentenceChrF(vocab, n, beta, ignored, join)
    for t_hyp, t_ref, bsz, first in C.REWARD_SHAPES:
        refs, hyps = C.batch(t_hyp, t_ref, bsz, first)
        want, _ = C.batch_scores(refs, hyps, vocab.index_to_word, n, beta, ignored or (), join)
        got = chrf(refs, hyps)
        assert got.dtype == np.float32 and np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -23
        lengths |= {len(C.characters(col, vocab.index_to_word)) for col in list(refs.T) + list(hyps.T)}
    assert {0, 1, 3, 63, 64, 65} <= lengths              # the batches hold what their docstring promises


def test_the_fixed_points_of_the_reference():
    from neuralmonkey_amd.trainers import self_critical_objective as S
    chrf = S.SentenceChrF(C.vocabulary())
    full, empty = [C.AB, C.E_ACUTE, C.END, C.A], [C.END, C.A, C.A, C.A]
    refs, hyps = np.array([full, full, empty, empty]).T, np.array([full, empty, full, empty]).T
    assert chrf(refs, hyps).tolist() == [1.0, 0.0, 0.0, 1.0]
    assert S._char_ngrams(["a", "b", "a"], 4) == [{"a": 2, "b": 1}, {"ab": 1, "ba": 1}, {"aba": 1}, {}]
    assert chrf.counts(list("abab"), list("bab")) == ([3, 2, 1, 0, 0, 0], [3, 2, 1, 0, 0, 0], [4, 3, 2, 1, 0, 0])
    recall = (3 / 4 + 2 / 3) / 2                         # and the precision is 1
    assert S.SentenceChrF(C.vocabulary(), n=2, beta=3.0).score(list("abab"), list("bab")) == 10.0 * recall / (9.0 + recall)


@pytest.mark.parametrize("words,kw,text", [
    (C.WORDS, dict(n=0), "n = 0 outside 1..6"), (C.WORDS, dict(n=7), "n = 7 outside 1..6"),
    (C.WORDS, dict(beta=0.0), "beta = 0.0 is not above 0"), (C.WORDS, dict(beta=-1.0), "is not above 0"),
    (["a", ""], {}, "an empty word or a word with a space"), (["a b"], {}, "an empty word or a word with a space"),
    ([chr(0x4E00 + i) for i in range(65534)], {}, "distinct characters, the space included, are more than 65534"),
])
def test_the_constructor_refuses(words, kw, text):
    from neuralmonkey_amd.trainers.self_critical_objective import SentenceChrF
    from neuralmonkey_amd.vocabulary import Vocabulary
    with pytest.raises(ValueError, match=re.escape(text)):
        SentenceChrF(Vocabulary(words), **kw)


def test_the_character_table():
    from neuralmonkey_amd.trainers import self_critical_objective as S
    vocab = C.vocabulary()
    chrf = S.SentenceChrF(vocab, ignored_symbols=[" ", "@"], join_subwords=True)
    rows, chars, longest = chrf.table()
    assert rows.dtype == np.int32 and chars.dtype == np.uint16 and longest == 70
    kept = ["<pad>", "<s>", "</s>", "<unk>", "a", "ab", "bab", C.LONG, "bé", "日", "ab", "b"]      # "@" is ignored
    assert rows[:, 2].tolist() == [len(w) for w in kept] and np.array_equal(rows[:, 1], rows[:, 2])    # no tail is left
    assert rows[:, 0].tolist() == np.cumsum([0] + rows[:-1, 2].tolist()).tolist()
    glued = [w.endswith("@@") for w in vocab.index_to_word]
    assert rows[:, 3].tolist() == [S.CHRF_SPACE_DROPPED | (S.CHRF_GLUE if g else 0) for g in glued]
    text = "".join(kept)                                 # ids are dense, equal exactly where the code points are
    assert len(chars) == len(text) and S.CHRF_SPACE_ID not in chars and chars.max() == len(set(text))
    assert all((chars[i] == chars[j]) == (text[i] == text[j]) for i in range(len(text)) for j in range(i, len(text), 7))
    assert chrf.table()[0] is rows and S.SentenceChrF(vocab, 2, 3.0, ["@", " "], True).table()[0] is rows    # cached
    plain, joined = S.SentenceChrF(vocab).table(), S.SentenceChrF(vocab, join_subwords=True).table()
    assert plain[0][C.AB_GLUE, 1:].tolist() == [4, 4, 0] and joined[0][C.AB_GLUE, 1:].tolist() == [2, 4, S.CHRF_GLUE]
    assert np.array_equal(plain[1], joined[1]) and len(plain[1]) == len("".join(vocab.index_to_word))


def test_header_table_and_wrappers_agree():
    from neuralmonkey_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nmhip_chrf.h")).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(nm_[a-z0-9_]+)\s*\((.*?)\)\s*;", text, flags=re.S)}
    assert set(decl) == set(_lib.CHRF_SIGNATURES) == {"nm_chrf_max_chars", "nm_chrf_reward", "nm_chrf_pairwise"}
    for name, (res, args) in _lib.CHRF_SIGNATURES.items():
        want = [_lib.P if "*" in p else _lib.L if "int64_t" in p else ctypes.c_int32 if "int32_t" in p
                else ctypes.c_double if "double" in p else _lib.I for p in decl[name].split(",") if p.strip() != "void"]
        assert list(args) == want and res is (_lib.L if name == "nm_chrf_max_chars" else _lib.I), name
    assert callable(ops.chrf_reward) and callable(ops.chrf_pairwise) and callable(ops.chrf_max_chars)


BASE = {"nm_chrf_reward": dict(ref=64, ref_stride=5, T_ref=7, hyp=64, hyp_stride=5, T_hyp=9, B=5, end=2, rows=64, chars=64,
                              V=12, max_word_chars=70, n=6, beta=1.0, reward=64, counts=None),
        "nm_chrf_pairwise": dict(tok=64, t_stride=15, T=7, B=5, n_samples=3, end=2, rows=64, chars=64, V=12,
                                 max_word_chars=70, n=6, beta=1.0, U=64)}


@pytest.mark.parametrize("name,kw,text", [
    ("reward", dict(n=0), "order n 0 outside 1..6"), ("reward", dict(n=7), "order n 7 outside 1..6"),
    ("reward", dict(beta=0.0), "beta 0 is not above 0"), ("reward", dict(beta=-2.0), "beta -2 is not above 0"),
    ("reward", dict(hyp=None), "null pointer"), ("reward", dict(chars=None), "null pointer"),
    ("reward", dict(rows=72), "rows is not 16-byte aligned"), ("reward", dict(hyp_stride=4), "row stride 5 or 4 below B = 5"),
    ("reward", dict(T_hyp=224), "231 tokens of up to 70 characters and a space are more than the 16384"),
    ("pairwise", dict(n=7), "order n 7 outside 1..6"), ("pairwise", dict(beta=0.0), "beta 0 is not above 0"),
    ("pairwise", dict(n_samples=65, t_stride=5 * 65), "n_samples 65 outside 1..64"), ("pairwise", dict(U=None), "null pointer"),
    ("pairwise", dict(t_stride=14), "row stride 14 below B * n_samples = 15"),
    ("pairwise", dict(T=116), "232 tokens of up to 70 characters and a space are more than the 16384"),
    ("pairwise", dict(B=1 << 15, n_samples=64, t_stride=1 << 21), "wavefronts in one launch"),
])
def test_refused_before_any_launch(name, kw, text):
    from neuralmonkey_amd import _lib, build
    build.build(verbose=False)
    lib, name = _lib.load(), "nm_chrf_" + name
    assert lib.nm_chrf_max_chars() == 16384 and 230 * 71 <= 16384 < 231 * 71       # 230 tokens are the most at 70
    assert getattr(lib, name)(None, *dict(BASE[name], **kw).values()) == -1       # the pointers (64) are never dereferenced
    assert lib.nm_last_error().decode().startswith(name + ": ") and text in lib.nm_last_error().decode()
