"""The REINFORCE reward over subword pieces without a GPU: the per-vocabulary table and the host restatement of the
kernel's keys (trainers/rl_trainer.py: ``piece_table``, ``joined_word_keys``) against the reference's own join,
``" ".join(tokens).replace("@@ ", "").split(" ")`` (rl_trainer.py:110-111), on every column of
tests/golden/subword_reward/scores.npz and on a seeded sweep over vocabularies of odd tokens; which evaluators take the
joined route; the binding table of include/nmhip_subword.h with its refusals; the fixture against what the host
evaluators return and, where the reference tree is, against a fresh run of its generator."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from .test_reinforce_host import REF, ulps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "subword_reward", "scores.npz")
GENERATOR = os.path.join(ROOT, "tests", "golden", "make_subword_reward_golden.py")
PIECES = ["ab@@", "c", "a@@", "bc", "@@", "x@@", "y", "abc"]
SPECIAL = ["<pad>", "<s>", "</s>", "<unk>"]


class Words:
    """What the functions under test read of a vocabulary."""

    def __init__(self, words):
        self.index_to_word = list(words)

    def __len__(self):
        return len(self.index_to_word)


def python_join(words, column):
    """rl_trainer.py:99-111 on one column of indices."""
    kept = []
    for index in column:
        if words[index] in ("</s>", "<pad>"):
            break
        kept.append(words[index])
    return " ".join(kept).replace("@@ ", "").split(" ")


@pytest.fixture(scope="module")
def golden():
    return np.load(FIXTURE)


def cases(golden):
    return sorted({k.split("/")[0] for k in golden.files if "/" in k})


# ---- the fixture --------------------------------------------------------------------------------------------------------------
def test_fixture_holds_what_the_issue_asks_for(golden):
    assert os.path.getsize(FIXTURE) < 100 * 1024
    assert [str(w) for w in golden["vocabulary"]] == SPECIAL + PIECES
    assert cases(golden) == ["hand_made", "hand_made_long"] + sorted(
        "random_b{}_r{}_h{}".format(b, r, h) for b in (5, 67) for r, h in ((1, 3), (7, 9), (70, 130)))
    words = [str(w) for w in golden["vocabulary"]]
    for name in cases(golden):
        ref, hyp = golden[name + "/ref"], golden[name + "/hyp"]
        assert ref.dtype == hyp.dtype == np.int32 and ref.shape[1] == hyp.shape[1]
        assert 0 <= min(ref.min(), hyp.min()) and max(ref.max(), hyp.max()) < len(words)
        for kind in ("gleu", "bleu"):
            assert golden[name + "/" + kind].dtype == np.float32 and golden[name + "/" + kind].shape == (ref.shape[1],)
        if name.startswith("random"):
            _, b, r, h = name.split("_")
            assert ref.shape == (int(r[1:]), int(b[1:])) and hyp.shape == (int(h[1:]), int(b[1:]))
    several = nonzero = sentences = scored = 0
    for name in cases(golden):
        if not name.startswith("random"):
            continue
        for side in ("ref", "hyp"):
            for column in golden[name + "/" + side].T:
                cut = [words[i] in ("</s>", "<pad>") for i in column]
                kept = cut.index(True) if True in cut else len(column)
                sentences += 1
                several += kept > len(python_join(words, column))
        nonzero += int((golden[name + "/gleu"] > 0).sum())
        scored += golden[name + "/gleu"].size
    assert 3 * several >= sentences and 4 * nonzero >= scored, (several, sentences, nonzero, scored)
    # the hand-made corners, by what the reference's join makes of them
    ref, hyp = golden["hand_made/ref"], golden["hand_made/hyp"]
    joined = [(python_join(words, r), python_join(words, h)) for r, h in zip(ref.T, hyp.T)]
    assert (["abc", "abc"], ["abc", "abc"]) in joined                         # one word, different pieces
    assert any(len(r) == 1 and len(r[0]) > 4 and r[0].endswith("@@") and r == h for r, h in joined)   # continuation pieces only
    assert (["c", "ab@@"], ["c", "ab@@"]) in joined                           # a last kept "@@" before </s> / <pad>
    assert (["c"] * 5 + ["ab@@"], ["c"] * 5 + ["ab@@"]) in joined             # ... at the end of the array
    assert (["@@"], ["@@"]) in joined and ([""], [""]) in joined
    assert any(r == [""] and h != [""] for r, h in joined) and any(h == [""] and r != [""] for r, h in joined)
    gleu = golden["hand_made/gleu"]
    assert gleu[joined.index((["abc", "abc"], ["abc", "abc"]))] == 1.0
    ref, hyp = golden["hand_made_long/ref"], golden["hand_made_long/hyp"]
    assert ref.shape[0] == 70 and hyp.shape[0] == 130
    assert words[ref[63, 0]] == "ab@@" and words[ref[64, 0]] == "c"           # a word over the positions 63 | 64
    assert all(words[i] == "a@@" for i in ref[60:67, 2]) and words[ref[67, 2]] == "bc"
    assert python_join(words, ref[:, 3]) == ["a" * 69 + "a@@"]                # one word of 70 pieces


def test_host_evaluators_reproduce_the_fixture(golden):
    from neuralmonkey_amd.evaluators.bleu import BLEUEvaluator
    from neuralmonkey_amd.evaluators.gleu import GLEUEvaluator
    from neuralmonkey_amd.trainers.rl_trainer import score_on_the_host
    vocab = Words(str(w) for w in golden["vocabulary"])
    for name in cases(golden):
        ref, hyp = golden[name + "/ref"], golden[name + "/hyp"]
        assert np.array_equal(score_on_the_host(vocab, GLEUEvaluator(), ref, hyp), golden[name + "/gleu"]), name
        assert ulps(score_on_the_host(vocab, BLEUEvaluator(), ref, hyp), golden[name + "/bleu"]).max() <= 1, name


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not here")
def test_regenerating_the_fixture_reproduces_it(golden, tmp_path):
    subprocess.run([sys.executable, GENERATOR, str(tmp_path)], check=True, cwd=ROOT, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    again = np.load(os.path.join(str(tmp_path), "scores.npz"))
    assert sorted(again.files) == sorted(golden.files)
    for key in golden.files:
        assert again[key].dtype == golden[key].dtype and np.array_equal(again[key], golden[key]), key


# ---- the table and the keys ---------------------------------------------------------------------------------------------------
def test_keys_of_every_fixture_column_are_the_keys_of_the_joined_strings(golden):
    from neuralmonkey_amd.trainers.rl_trainer import joined_word_keys, word_key
    vocab = Words(str(w) for w in golden["vocabulary"])
    key_of = {}
    for name in cases(golden):
        for side in ("ref", "hyp"):
            for column in golden[name + "/" + side].T:
                strings = python_join(vocab.index_to_word, column)
                keys = joined_word_keys(vocab, [int(i) for i in column])
                assert keys == [word_key(w) for w in strings], (name, side, strings)
                for word, key in zip(strings, keys):
                    assert key_of.setdefault(key, word) == word           # no two distinct words of the fixture share a key
    assert len(key_of) > 100 and key_of[(0, 0, 0)] == ""


def test_keys_on_a_sweep_over_odd_tokens():
    from neuralmonkey_amd.trainers.rl_trainer import joined_word_keys, piece_table, word_key
    odd = SPECIAL + ["@@", "@", "a@", "@@@", "a@@@", "@@@@", "a@@b", "a", "b@@", "a", "</s>", "é@@", "日本",
                     "<pad>@@", "@@a"]
    vocab = Words(odd)
    table = piece_table(vocab)
    assert table.shape == (len(odd), 12) and table.dtype == np.int32 and table.min() >= 0
    assert [i for i, row in enumerate(table) if row[10] & 2] == [0, 2, odd.index("</s>", 3)]    # the cut is by STRING
    assert [odd[i] for i, row in enumerate(table) if row[10] & 1] == [w for w in odd if w.endswith("@@")]
    assert tuple(table[odd.index("@@")][0:5]) == (0, 0, 1, 1, 0)              # the empty stem: the identity
    assert table[odd.index("é@@")][4] == 2 and table[odd.index("日本")][9] == 6   # lengths in UTF-8 bytes
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(4000):
        column = [int(i) for i in rng.integers(0, len(odd), int(rng.integers(0, 9)))]
        strings = python_join(odd, column)
        assert joined_word_keys(vocab, column) == [word_key(w) for w in strings], (column, strings)
        seen.update(strings)
    assert "" in seen and "@@" in seen and len(seen) > 200
    assert len({word_key(w) for w in seen}) == len(seen)                      # no collision among them
    assert joined_word_keys(vocab, [7, len(odd), 7]) == [word_key("@@@")]     # an id outside the table cuts
    assert joined_word_keys(vocab, [-1, 7]) == [(0, 0, 0)]


def test_hash_is_composable_and_a_table_needs_proper_words():
    from neuralmonkey_amd.trainers import rl_trainer as R
    rng = np.random.default_rng(6)
    for _ in range(200):
        s, t, u = ("".join(chr(int(c)) for c in rng.integers(33, 0x2fff, int(rng.integers(0, 12)))) for _ in range(3))
        hs, ht, hu = R._piece_element(s), R._piece_element(t), R._piece_element(u)
        assert R._compose(hs, ht) == R._piece_element(s + t)
        assert R._compose(R._compose(hs, ht), hu) == R._compose(hs, R._compose(ht, hu)) == R._piece_element(s + t + u)
        assert R._compose((0, 0, 1, 1, 0), hs) == hs == R._compose(hs, (0, 0, 1, 1, 0))
    for modulus, base in zip(R.PIECE_MODULI, R.PIECE_BASES):
        assert 1 << 30 < modulus < 1 << 31 and 256 < base < modulus
        assert all(modulus % d for d in range(2, int(modulus ** 0.5) + 1))       # prime
    assert R.PIECE_MODULI[0] != R.PIECE_MODULI[1] and R.PIECE_MODULI[0] * R.PIECE_MODULI[1] > 1 << 60
    assert R.piece_table(Words(SPECIAL + ["a", ""])) is None
    assert R.piece_table(Words(SPECIAL + ["a b", "c"])) is None
    grown = Words(SPECIAL + PIECES)
    first = R.piece_table(grown)
    assert R.piece_table(grown) is first                                       # computed once ...
    grown.index_to_word.append("z@@")
    assert R.piece_table(grown) is not first and len(R.piece_table(grown)) == 13     # ... per size of the vocabulary


# ---- which rewards take the joined route ----------------------------------------------------------------------------------------
def test_evaluator_conditions_of_the_joined_route(tmp_path_factory):
    import tarfile
    from neuralmonkey_amd.evaluators.bleu import BLEUEvaluator
    from neuralmonkey_amd.evaluators.gleu import GLEUEvaluator
    from neuralmonkey_amd.trainers.rl_trainer import ReinforceObjective
    from neuralmonkey_amd.vocabulary import Vocabulary
    from .test_reference_inis import BUNDLE as DATA_BUNDLE, load_verbatim
    from .test_reinforce_host import BUNDLE
    root = tmp_path_factory.mktemp("reference_tests_rl_pieces")
    for bundle in (DATA_BUNDLE, BUNDLE):
        with tarfile.open(bundle) as tar:
            tar.extractall(root)
    dec = load_verbatim(str(root), "rl", initialize=False, device="cpu").runners[0].decoder
    whole = ReinforceObjective(dec, GLEUEvaluator())
    assert whole.device_reward() == ("gleu", 4) == whole.joined_device_reward()   # (rewards() tries device_reward first)
    dec.vocabulary = Vocabulary(list(PIECES))                                  # the same decoder over BPE pieces
    assert list(dec.vocabulary.index_to_word) == SPECIAL + PIECES
    assert ReinforceObjective(dec, GLEUEvaluator()).device_reward() is None
    assert ReinforceObjective(dec, GLEUEvaluator()).joined_device_reward() == ("gleu", 4)
    assert ReinforceObjective(dec, BLEUEvaluator(n=2)).joined_device_reward() == ("bleu", 2)
    for host_side in (GLEUEvaluator(deduplicate=True), BLEUEvaluator(multiple_references_separator="|"),
                      GLEUEvaluator(n=5), lambda hyp, ref: 0.0):
        objective = ReinforceObjective(dec, host_side)
        assert objective.device_reward() is None and objective.joined_device_reward() is None
    dec.vocabulary = Words(SPECIAL + ["a b"])                                  # no table: the host
    assert ReinforceObjective(dec, GLEUEvaluator()).joined_device_reward() is None


# ---- the binding table ----------------------------------------------------------------------------------------------------------
def subword_header_symbols():
    text = open(os.path.join(ROOT, "include", "nmhip_subword.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nm_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


def test_subword_header_matches_its_binding_table(lib):
    from neuralmonkey_amd import _lib
    from .test_abi import header_symbols
    from .test_cnn2d_host import image_header_symbols
    from .test_convs2s_host import convs2s_header_symbols
    from .test_ctc_host import ctc_header_symbols
    from .test_labeler_host import label_header_symbols
    from .test_pool_host import pool_header_symbols
    from .test_reinforce_host import rl_header_symbols
    from .test_self_critical_host import reward_header_symbols
    mine = subword_header_symbols()
    assert mine == set(_lib.SUBWORD_SIGNATURES) == {"nm_eval_joined_sentence_score",
                                                     "nm_eval_joined_sentence_score_max_tokens"}
    for other in (_lib.SIGNATURES, _lib.CTC_SIGNATURES, _lib.LABEL_SIGNATURES, _lib.POOL_SIGNATURES, _lib.CONVS2S_SIGNATURES,
                  _lib.IMAGE_SIGNATURES, _lib.REWARD_SIGNATURES, _lib.RL_SIGNATURES, _lib.GRU_SEQ_SIGNATURES):
        assert not mine & set(other)
    for theirs in (header_symbols, ctc_header_symbols, label_header_symbols, pool_header_symbols, convs2s_header_symbols,
                   image_header_symbols, reward_header_symbols, rl_header_symbols):
        assert not mine & theirs()
    for name, (res, args) in _lib.SUBWORD_SIGNATURES.items():
        fn = getattr(lib, name)                                          # exported, and bound by load()
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    header = open(os.path.join(ROOT, "include", "nmhip_subword.h")).read()
    for cited in ("rl_trainer.py:83-115", ":110-111", "gleu.py:47-110", "bleu.py:98-133,196-236", "bleu.py:122-124",
                  "gleu.py:80-82", "bleu.py:212-236"):
        assert cited in header, cited                                    # the lines it replaces
    for said in ("(length in bytes, hash modulo M1, hash modulo M2)", "NOT EXACT BY CONSTRUCTION", "per comparison",
                 "outside [0, V)"):
        assert said in header, said


def test_entry_points_refuse_before_any_launch(lib):
    """Host buffers and a null stream: a call that got as far as a launch would fault or fail differently."""
    ints = (ctypes.c_int32 * 4096)()
    floats = (ctypes.c_float * 4096)()
    assert lib.nm_eval_joined_sentence_score_max_tokens() == 8192 >= 4096

    def score(kind=1, order=4, ref=ints, rs=5, t_ref=7, hyp=ints, hs=5, t_hyp=9, b=5, table=ints, rows=12, v=12,
              out=floats):
        return lib.nm_eval_joined_sentence_score(None, kind, order, ref, rs, t_ref, hyp, hs, t_hyp, b, table, rows, v, out)
    name = b"nm_eval_joined_sentence_score: "
    for kwargs, text in (
            (dict(kind=2), b"kind 2 (0 BLEU, 1 GLEU)"), (dict(kind=-1), b"kind -1 (0 BLEU, 1 GLEU)"),
            (dict(order=0), b"order 0 outside 1..4"), (dict(order=5), b"order 5 outside 1..4"),
            (dict(b=-1), b"bad sizes B -1, T_ref 7, T_hyp 9"), (dict(t_ref=0), b"bad sizes B 5, T_ref 0, T_hyp 9"),
            (dict(t_hyp=0), b"bad sizes B 5, T_ref 7, T_hyp 0"),
            (dict(t_ref=8000, t_hyp=193), b"T_ref 8000 + T_hyp 193 tokens above the 8192 the LDS staging holds"),
            (dict(t_hyp=1 << 40), b"T_ref 7 + T_hyp 1099511627776 tokens above the 8192 the LDS staging holds"),
            (dict(rs=4), b"row strides 4, 5 below B 5"), (dict(hs=4), b"row strides 5, 4 below B 5"),
            (dict(rs=1 << 30), b"a token array spans more than 2^31 - 1 elements"),
            (dict(v=0), b"vocabulary size 0"), (dict(v=1 << 31, rows=1 << 31), b"vocabulary size 2147483648"),
            (dict(rows=11), b"a table of 11 rows for a vocabulary of 12"),
            (dict(ref=None), b"null pointer"), (dict(hyp=None), b"null pointer"), (dict(table=None), b"null pointer"),
            (dict(out=None), b"null pointer")):
        assert score(**kwargs) < 0 and lib.nm_last_error() == name + text, (kwargs, lib.nm_last_error())
    assert score(b=0, rs=0, hs=0, ref=None, hyp=None, table=None, out=None) == 0        # B == 0 is a no-op


def test_ledger_covers_the_header():
    from . import test_subword_reward_kernels_gpu as K
    from .test_pointwise_refs import ledger_problems
    assert ledger_problems(K.LEDGER, subword_header_symbols()) == []
    assert not [s for s, e in K.LEDGER.items() if isinstance(e, tuple)]      # every entry point names a test that calls it


def test_the_kernel_does_not_spill(lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_resources
    finally:
        sys.path.pop(0)
    mine = {k: v for k, v in kernel_resources().items() if "joined_score_kernel" in k}
    assert len(mine) == 1 and all(v["scratch"] == 0 for v in mine.values()), mine
