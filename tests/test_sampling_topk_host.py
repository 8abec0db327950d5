"""Truncated sampling without a GPU: the entry point in its header and binding table, every argument the entry refuses
(all before a launch, so no device is needed), the bounds of SamplingDecoder and SamplingRunner, the runner range, and
an INI text that names the new classes by their short and full paths."""
import ctypes
import os
import re

import pytest

from . import sampling_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nmhip_sample.h")


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(nm_[a-z0-9_]+)\s*\((.*?)\)\s*;", text, flags=re.S)}


def test_sample_header_matches_its_binding_table():
    from neuralmonkey_amd import _lib, ops
    decl = _declarations()
    assert set(decl) == set(_lib.SAMPLE_SIGNATURES) == {"nm_sample_step", "nm_sample_lds_max_columns"}
    params = decl["nm_sample_step"].split(",")
    res, args = _lib.SAMPLE_SIGNATURES["nm_sample_step"]
    assert res is _lib.I and len(params) == len(args) == 23           # one entry of the table per parameter
    for p, a in zip(params, args):
        want = (_lib.P if "*" in p else _lib.L if "int64_t" in p else _lib.F if "float" in p
                else ctypes.c_uint32 if "uint32_t" in p else _lib.I)
        assert a is want, p
    assert decl["nm_sample_lds_max_columns"].strip() == "void"
    assert _lib.SAMPLE_SIGNATURES["nm_sample_lds_max_columns"] == (_lib.L, [])
    assert callable(ops.sample_step)
    # the companion header leaves the main one and its table alone
    assert not set(_lib.SAMPLE_SIGNATURES) & set(_lib.SIGNATURES)
    assert "nm_sample" not in open(os.path.join(ROOT, "include", "nmhip.h")).read()


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


def test_the_symbols_are_exported_and_the_lds_limit_is_the_tables(lib):
    assert hasattr(lib, "nm_sample_step") and hasattr(lib, "nm_sample_lds_max_columns")
    assert int(lib.nm_sample_lds_max_columns()) == SC.LDS_MAX
    assert SC.LDS_MAX * 4 + 8 * 1024 <= 160 * 1024                     # the row and the histograms fit a CU's LDS


def _call(lib, **kw):
    """nm_sample_step on pointers that are never dereferenced: a refusal comes before any launch."""
    a = dict(logits=64, ldx=10, rows=2, V=10, inv_t=1.0, top_k=0, top_p=1.0, salt=64, step=0, end=2, fin=64, lps=64,
             lens=64, sym=64, lp=64, kept=64, ofin=64, olps=64, olens=64, allfin=None, ws=None, ws_bytes=0)
    a.update(kw)
    return lib.nm_sample_step(None, a["logits"], a["ldx"], a["rows"], a["V"], a["inv_t"], a["top_k"], a["top_p"],
                              a["salt"], a["step"], a["end"], a["fin"], a["lps"], a["lens"], a["sym"], a["lp"],
                              a["kept"], a["ofin"], a["olps"], a["olens"], a["allfin"], a["ws"], a["ws_bytes"])


@pytest.mark.parametrize("kw,text", [
    (dict(logits=None), "null input"), (dict(salt=None), "null input"), (dict(fin=None), "null input"),
    (dict(lps=None), "null input"), (dict(lens=None), "null input"),
    (dict(sym=None), "null output"), (dict(lp=None), "null output"), (dict(kept=None), "null output"),
    (dict(ofin=None), "null output"), (dict(olps=None), "null output"), (dict(olens=None), "null output"),
    (dict(top_p=0.0), "top_p"), (dict(top_p=1.5), "top_p"), (dict(top_p=float("nan")), "top_p"),
    (dict(top_k=-1), "top_k"),
    (dict(inv_t=0.0), "inv_temperature"), (dict(inv_t=float("inf")), "inv_temperature"),
    (dict(inv_t=-1.0), "inv_temperature"), (dict(inv_t=float("nan")), "inv_temperature"),
    (dict(ldx=9), "ldx"), (dict(V=0, ldx=0), "V ="), (dict(V=1 << 30, ldx=1 << 30), "V ="), (dict(rows=-1), "rows"),
    (dict(ws_bytes=-4), "workspace"),
])
def test_argument_errors_return_a_code_and_a_text(lib, kw, text):
    assert _call(lib, **kw) == -1
    assert text in lib.nm_last_error().decode()


def test_no_rows_is_not_an_error(lib):
    assert _call(lib, rows=0) == 0


def _model():
    from neuralmonkey_amd import synthetic
    return synthetic.build_translation_model(vocab_src=30, vocab_tgt=40, emb=8, rnn=8, max_len=6, beam_size=0,
                                             max_steps=4, device="cpu")


def test_constructor_bounds():
    from neuralmonkey_amd.decoders import SamplingDecoder
    m = _model()
    make = lambda **kw: SamplingDecoder(name="s", parent_decoder=m.decoder, max_steps=kw.pop("max_steps", 4), **kw)
    d = make(num_samples=64, temperature=0.7, top_k=40, top_p=0.9)
    assert (d.num_samples, d.temperature, d.top_k, d.top_p, d.max_steps_int) == (64, 0.7, 40, 0.9, 4)
    assert d.vocabulary is m.decoder.vocabulary and d.parent_decoder is m.decoder
    d = make()
    assert (d.num_samples, d.temperature, d.top_k, d.top_p) == (1, 1.0, 0, 1.0)
    for n in (0, 65):
        with pytest.raises(ValueError, match="rows_per_key <= 64"):
            make(num_samples=n)
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5),
               dict(max_steps=0)):
        with pytest.raises(ValueError):
            make(**kw)
    with pytest.raises(TypeError, match="parent_decoder"):
        SamplingDecoder(name="s", parent_decoder=d, max_steps=4)       # not an autoregressive decoder
    from neuralmonkey_amd.decoders.autoregressive import AutoregressiveDecoder
    assert not hasattr(AutoregressiveDecoder, "make_stepper")
    bare = object.__new__(AutoregressiveDecoder)                       # a parent without a stepwise interface
    with pytest.raises(NotImplementedError, match="make_stepper"):
        SamplingDecoder(name="s", parent_decoder=bare, max_steps=4)
    with pytest.raises(TypeError):
        make(num_samples="3")
    with pytest.raises(NotImplementedError, match="ensemble"):
        d.ensemble_outputs([object(), object()])


def test_runner_bounds_and_range_names():
    from neuralmonkey_amd.decoders import SamplingDecoder
    from neuralmonkey_amd.runners import SamplingRunner, sampling_runner_range
    m = _model()
    d = SamplingDecoder(name="s", parent_decoder=m.decoder, max_steps=4, num_samples=5, top_k=3)
    r = SamplingRunner("target_sample", d, sample=5)
    assert r.sample == 5 and r.loss_names == ["sample_logprob"] and r.decoder is d
    assert set(r.fetches) == {"samples"} and r.ahead_fetches()
    assert {d, m.decoder, m.encoder} <= set(r.feedables)
    for bad in (0, 6):
        with pytest.raises(ValueError, match="between 1 and the number of samples"):
            SamplingRunner("target_sample", d, sample=bad)
    runners = sampling_runner_range("target_sample", d, max_sample=3)
    assert [x.output_series for x in runners] == ["target_sample.sample{:03d}".format(i) for i in (1, 2, 3)]
    assert [x.sample for x in runners] == [1, 2, 3]
    assert len(sampling_runner_range("target_sample", d)) == 5
    with pytest.raises(ValueError):
        sampling_runner_range("target_sample", d, max_sample=6)
    with pytest.raises(NotImplementedError, match="ensemble"):
        r.get_executable(compute_losses=False, summaries=False, num_sessions=2)


SAMPLING_INI = """
[main]
name="sampling"
batch_size=4
epochs=1
train_dataset=<train_data>
runners=[<sample_one>, <sample_range>]
[train_data]
class=dataset.load
series=["source", "target"]
data=["{src}", "{tgt}"]
[vocabulary]
class=vocabulary.from_wordlist
path="{vocab}"
[encoder]
class=encoders.SentenceEncoder
rnn_size=6
max_input_len=5
embedding_size=8
data_id="source"
vocabulary=<vocabulary>
[attention]
class=attention.Attention
encoder=<encoder>
[decoder]
class=decoders.Decoder
encoders=[<encoder>]
attentions=[<attention>]
rnn_size=8
embedding_size=8
data_id="target"
max_output_len=5
vocabulary=<vocabulary>
[sampler]
class=decoders.sampling_decoder.SamplingDecoder
parent_decoder=<decoder>
max_steps=5
num_samples=3
temperature=0.8
top_k=4
top_p=0.9
[short_sampler]
class=decoders.SamplingDecoder
parent_decoder=<decoder>
max_steps=5
[sample_one]
class=runners.SamplingRunner
decoder=<short_sampler>
output_series="target_one"
[sample_range]
class=runners.sampling_runner.sampling_runner_range
decoder=<sampler>
output_series="target_sample"
max_sample=2
"""


def test_ini_text_with_the_short_and_the_full_paths_builds(tmp_path):
    """Fails on a tree without the feature with SymbolNotShipped."""
    from neuralmonkey_amd.config.configuration import load_experiment
    from neuralmonkey_amd.decoders import Decoder, SamplingDecoder
    from neuralmonkey_amd.runners import SamplingRunner
    (tmp_path / "src.txt").write_text("a b c\nb c\nc a a b\na\n")
    (tmp_path / "tgt.txt").write_text("x y\ny\nx x y\ny y\n")
    (tmp_path / "vocab.tsv").write_text("Word\tCount\n<pad>\t1\n<s>\t1\n</s>\t1\n<unk>\t1\n"
                                        "a\t9\nb\t8\nc\t7\nx\t6\ny\t5\n")
    path = tmp_path / "sampling.ini"
    path.write_text(SAMPLING_INI.format(src=tmp_path / "src.txt", tgt=tmp_path / "tgt.txt",
                                        vocab=tmp_path / "vocab.tsv"))
    model = load_experiment(str(path), device="cpu", seed=4321)
    one, first, second = model.runners
    assert all(isinstance(r, SamplingRunner) for r in model.runners)
    assert [r.output_series for r in model.runners] == ["target_one", "target_sample.sample001", "target_sample.sample002"]
    assert isinstance(one.decoder, SamplingDecoder) and one.decoder is not first.decoder and first.decoder is second.decoder
    s = first.decoder
    assert (s.num_samples, s.temperature, s.top_k, s.top_p, s.max_steps_int) == (3, 0.8, 4, 0.9, 5)
    assert isinstance(s.parent_decoder, Decoder) and s.parent_decoder is one.decoder.parent_decoder
    assert (one.decoder.num_samples, one.decoder.top_k, one.decoder.top_p) == (1, 0, 1.0)
