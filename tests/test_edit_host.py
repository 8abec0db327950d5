"""The edit-distance scores without a GPU: the two NumPy functions on hand-computed cases, the entry points in their
header, binding table and wrappers, and the arguments they refuse (before a launch, so no device is needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# reference and hypothesis columns (</s> is 2), then accuracy and negative WER by hand from d, lr, lh
HAND = [
    ([5, 6, 7, 2, 0, 0, 0], [5, 7, 2, 0, 0, 0, 0], 1 - 1 / 3, -1 / 3),     # one deletion: d 1, lr 3, lh 2
    ([3, 4, 5, 5, 6, 7, 2], [8, 4, 5, 5, 4, 7, 9], 1 - 3 / 7, -3 / 6),     # kitten | sitting, the hypothesis never ends
    ([2, 5, 5, 5, 5, 5, 5], [2, 0, 0, 0, 0, 0, 0], 1, 0),                  # both empty
    ([2, 0, 0, 0, 0, 0, 0], [5, 6, 2, 0, 0, 0, 0], 0, -2),                 # an empty reference: d 2
    ([5, 6, 7, 2, 0, 0, 0], [2, 6, 7, 0, 0, 0, 0], 0, -1),                 # an empty hypothesis: d 3
    ([5, 0, 0, 0, 0, 0, 0], [5, 2, 0, 0, 0, 0, 0], 1 - 6 / 7, -6 / 7),     # no end token: <pad> is a token, lr 7
    ([4, 3, 4, 2, 0, 0, 0], [4, 3, 4, 2, 9, 9, 9], 1, 0),                  # identical sentences
]


def test_the_numpy_functions_on_hand_computed_cases():
    from neuralmonkey_amd.trainers import self_critical_objective as S
    refs, hyps = (np.array([case[k] for case in HAND]).T for k in (0, 1))
    accuracy = S.sentence_edit_accuracy(refs, hyps.astype(np.int32))
    assert accuracy.tobytes() == np.float32([case[2] for case in HAND]).tobytes()
    assert S.sentence_neg_wer(refs, hyps).tobytes() == np.float32([case[3] for case in HAND]).tobytes()
    assert S.sentence_edit_accuracy(hyps, refs).tobytes() == accuracy.tobytes()           # symmetric


def test_header_table_and_wrappers_agree():
    from neuralmonkey_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nmhip_edit.h")).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(nm_[a-z0-9_]+)\s*\((.*?)\)\s*;", text, flags=re.S)}
    assert set(decl) == set(_lib.EDIT_SIGNATURES) == {"nm_edit_max_tokens", "nm_edit_reward", "nm_edit_pairwise"}
    for name, (res, args) in _lib.EDIT_SIGNATURES.items():
        want = [_lib.P if "*" in p else _lib.L if "int64_t" in p else ctypes.c_int32 if "int32_t" in p else _lib.I
                for p in decl[name].split(",") if p.strip() != "void"]
        assert list(args) == want and res is (_lib.L if name == "nm_edit_max_tokens" else _lib.I), name
    assert callable(ops.edit_reward) and callable(ops.edit_pairwise) and callable(ops.edit_max_tokens)


REWARD = dict(kind=0, ref=64, ref_stride=5, T_ref=7, hyp=64, hyp_stride=5, T_hyp=9, B=5, end=2, reward=64, dist=None)
PAIRWISE = dict(kind=1, tok=64, t_stride=15, T=7, B=5, n=3, end=2, U=64)


@pytest.mark.parametrize("name,base,kw,text", [
    ("nm_edit_reward", REWARD, dict(T_hyp=1025), "T_ref 7 or T_hyp 1025 above the 1024 tokens"),
    ("nm_edit_reward", REWARD, dict(kind=2), "kind 2"), ("nm_edit_reward", REWARD, dict(hyp=None), "null pointer"),
    ("nm_edit_reward", REWARD, dict(hyp_stride=4), "row stride 5 or 4 below B = 5"),
    ("nm_edit_pairwise", PAIRWISE, dict(T=1025), "T 1025 above the 1024 tokens"),
    ("nm_edit_pairwise", PAIRWISE, dict(n=65, t_stride=5 * 65), "n 65 samples outside 1..64"),
    ("nm_edit_pairwise", PAIRWISE, dict(t_stride=14), "row stride 14 below B * n = 15"),
    ("nm_edit_pairwise", PAIRWISE, dict(U=None), "null pointer"),
    ("nm_edit_pairwise", PAIRWISE, dict(B=1 << 18, n=64, t_stride=1 << 24), "wavefronts in one launch"),
])
def test_refused_before_any_launch(name, base, kw, text):
    from neuralmonkey_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert getattr(lib, name)(None, *dict(base, **kw).values()) == -1       # the pointers (64) are never dereferenced
    assert lib.nm_last_error().decode().startswith(name + ": ") and text in lib.nm_last_error().decode()
