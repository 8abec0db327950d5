"""The fixtures of the supervised-attention tests, made where the reference tree is:

    python tests/golden/make_alignment_fixture.py

* tests/golden/reference_tests_alignment.tar.gz -- tests/alignment.ini and tests/data/train.tc.ali, the reference's bytes
  (the parallel text and the vocabularies the configuration names are in reference_tests.tar.gz), bundled the way
  make_reference_ini_fixture.py bundles its archives: configs and data only, no reference source code;
* tests/golden/alignment_preprocessor.npz -- what the REFERENCE'S WordAlignmentPreprocessor (pure NumPy, loaded from
  its file and run here) returns for the first 32 lines of train.tc.ali with the configuration's sizes, and for the
  hand-written lines of ``CASES`` below: both separators, weights, one-based indices, no normalisation, pairs outside
  the matrix.  Arrays and the lines that produced them, not code;
* tests/golden/alignment_signatures.json -- the constructor parameters of the three classes, read from the reference's
  source as tests/test_reference_signatures.py reads them."""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_reference_ini_fixture import REF, members, write  # noqa: E402  pylint: disable=wrong-import-position

OUT = os.path.join(HERE, "reference_tests_alignment.tar.gz")
OUT_NPZ = os.path.join(HERE, "alignment_preprocessor.npz")
OUT_SIGNATURES = os.path.join(HERE, "alignment_signatures.json")
LINES = 32

# name -> (constructor arguments, sentences)
CASES = {
    "colon_and_dash": (dict(source_len=5, target_len=4), ["0:0 1-1 2:1 4-3", "3:2", ""]),
    "weights": (dict(source_len=5, target_len=4), ["0-0/0.5 1-0/0.25 2:1/2 3:3/0.5 4-3", "0-2/0 1-2/0"]),
    "one_based": (dict(source_len=4, target_len=3, zero_based=False), ["1-1 2-2 3:3 4-3/0.5", "4-1 1:3"]),
    "not_normalized": (dict(source_len=4, target_len=3, normalize=False), ["0-0 1-0 2-1/0.5 3:2/3", "0-1/0.125"]),
    "not_normalized_float64": (dict(source_len=3, target_len=2, normalize=False, dtype="float64"), ["0-0/0.1 2:1/0.7"]),
    "out_of_range": (dict(source_len=3, target_len=2), ["0-0 3-0 2-2 5:7 1-1 2-1", "3-2 4-4"]),
    "one_based_out_of_range": (dict(source_len=3, target_len=2, zero_based=False), ["1-1 4-1 3-3 3-2 2:2/0.5"]),
}

SIGNATURES = [("decoders/word_alignment_decoder.py", "WordAlignmentDecoder"),
              ("runners/word_alignment_runner.py", "WordAlignmentRunner"),
              ("processors/alignment.py", "WordAlignmentPreprocessor")]


def build(kwargs, module):
    kwargs = dict(kwargs)
    if "dtype" in kwargs:
        kwargs["dtype"] = getattr(np, kwargs["dtype"])
    return module.WordAlignmentPreprocessor(**kwargs)


def main():
    write(OUT, members(["alignment"], ["train.tc.ali"]))
    spec = importlib.util.spec_from_file_location(
        "reference_alignment", os.path.join(REF, "neuralmonkey", "processors", "alignment.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    with open(os.path.join(REF, "tests", "data", "train.tc.ali"), encoding="utf-8") as handle:
        lines = [line.rstrip("\n") for _, line in zip(range(LINES), handle)]
    arrays = {"ini/lines": np.asarray(lines),
              "ini/out": np.stack([build(dict(source_len=12, target_len=8), module)(line.split()) for line in lines])}
    for name, (kwargs, sentences) in CASES.items():
        arrays[name + "/args"] = np.asarray(json.dumps(kwargs, sort_keys=True))
        arrays[name + "/lines"] = np.asarray(sentences)
        arrays[name + "/out"] = np.stack([build(kwargs, module)(s.split()) for s in sentences])
    np.savez_compressed(OUT_NPZ, **arrays)
    print(OUT_NPZ, os.path.getsize(OUT_NPZ))
    from tests.test_reference_signatures import read_reference_parameters
    listed = {}
    for path, name in SIGNATURES:
        listed.setdefault(path, {})[name] = read_reference_parameters(path, name)
    with open(OUT_SIGNATURES, "w", encoding="utf-8") as handle:
        json.dump(listed, handle, indent=1)
        handle.write("\n")
    print(OUT_SIGNATURES)


if __name__ == "__main__":
    main()
