"""Wide beams (17 to 64 hypotheses) on the host side: the constructor's bound, the runners over a wide beam, the
workspace size of the narrow kernels (unchanged), and the new entry point in its header and binding table."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(beam):
    from neuralmonkey_amd import synthetic
    return synthetic.build_translation_model(vocab_src=30, vocab_tgt=40, emb=8, rnn=8, max_len=6, beam_size=beam,
                                             max_steps=4, device="cpu")


@pytest.mark.parametrize("beam", [17, 32, 64])
def test_wide_beam_decoder_constructs(beam):
    from neuralmonkey_amd.runners import BeamSearchRunner
    m = _model(beam)
    assert m.beam_decoder.beam_size == beam
    assert BeamSearchRunner("target_beam", m.beam_decoder, rank=beam).rank == beam
    with pytest.raises(ValueError):
        BeamSearchRunner("target_beam", m.beam_decoder, rank=beam + 1)


@pytest.mark.parametrize("beam", [0, 65])
def test_beam_sizes_outside_1_to_64_are_refused(beam):
    from neuralmonkey_amd.decoders import BeamSearchDecoder
    m = _model(2)
    with pytest.raises(ValueError, match="between 1 and 64"):
        BeamSearchDecoder(name="too_wide", parent_decoder=m.decoder, beam_size=beam, max_steps=4,
                          length_normalization=0.6)


def test_runner_range_over_a_wide_beam():
    from neuralmonkey_amd.runners import beam_search_runner_range
    m = _model(32)
    runners = beam_search_runner_range("target_beam", m.beam_decoder, max_rank=20)
    assert [r.output_series for r in runners] == ["target_beam.rank{:03d}".format(i) for i in range(1, 21)]
    assert [r.rank for r in runners] == list(range(1, 21))
    assert len(beam_search_runner_range("target_beam", m.beam_decoder)) == 32
    with pytest.raises(ValueError):
        beam_search_runner_range("target_beam", m.beam_decoder, max_rank=33)


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "nmhip_beam_wide.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nm_[a-z0-9_]+)\s*\(", text))


def test_beam_wide_header_matches_its_binding_table():
    from neuralmonkey_amd import _lib, ops
    assert _header_symbols() == set(_lib.BEAM_WIDE_SIGNATURES) == {"nm_beam_topk_step_wide"}
    # one argument of the table per parameter of the declaration
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nmhip_beam_wide.h")).read(), flags=re.S)
    params = re.search(r"nm_beam_topk_step_wide\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
    res, args = _lib.BEAM_WIDE_SIGNATURES["nm_beam_topk_step_wide"]
    assert len(params) == len(args) == 27
    for p, a in zip(params, args):
        want = _lib.P if "*" in p else (_lib.L if "int64_t" in p else _lib.I)
        assert a is want, p
    assert callable(ops.beam_topk_step_wide)


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


def test_the_symbol_is_exported_and_the_narrow_workspace_keeps_its_size(lib):
    assert hasattr(lib, "nm_beam_topk_step_wide")
    for k in (1, 4, 8, 16):
        for b, v in ((1, 5), (3, 1000), (128, 32000)):
            assert int(lib.nm_beam_workspace_bytes(b, k, v)) == b * 64 * 16 * 8 + 256
    # a wide beam needs room for its lists and candidates; the size grows with the sentences, not with V beyond 8 slices
    assert int(lib.nm_beam_workspace_bytes(128, 64, 32000)) > 128 * 64 * 16 * 8 + 256
    assert int(lib.nm_beam_workspace_bytes(2, 64, 1 << 24)) == int(lib.nm_beam_workspace_bytes(2, 64, 1 << 20))
