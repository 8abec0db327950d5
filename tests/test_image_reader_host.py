"""The image reader without a GPU: the reference's class paths through the symbol resolver, the two readers' signatures,
every refusal with the reference's words, the PGM / PPM parser, and -- for every case of
tests/golden/image_reader_golden.npz -- the product's geometry and tables applied by the NumPy restatement of the two
passes (tests/image_reader_ref.py) against the array the reference's reader produced with Pillow: exact equality in all
three modes.  The fixture's cases (sources are width x height; synthetic ones have independent R, G and B):

  a  the reader of tests/str.ini (256 x 32, both sides rescaled, mode F): four of the reference's JPEGs, 1x1, 2x3 (the
     window clipped at both ends), 256x32 (the early return), 256x31 (vertical pass only), 300x32 (horizontal only,
     a downscale), 700x90 (both passes, more than 3 taps)
  b  target 40 x 20 in the modes L and RGB: 1 both sides, BILINEAR; 2 both sides with the aspect kept, BICUBIC, 53x37,
     200x20 and 3x50 (one column); 3 the width only (53x37 -> 40x27, an odd crop difference of 7); 4 the height only
     (-> 28x20, padded); 5 no rescaling (53x37: differences 13 and 17, 10x7: padded both ways, 41x20: difference 1);
     6 an L source to RGB and an RGB source to F
  c  target 300 x 5: an output row wider than a workgroup
  d  imagenet_reader, target 16 x 16, all four combinations of its two flags"""
import json
import os
import re
import sys
import tarfile
import warnings

import numpy as np
import pytest

from . import image_reader_ref as ref
from .test_reference_inis import REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = "readers/image_reader.py"


# ---- the public surface ----------------------------------------------------------------------------------------------------
def test_reference_class_paths_resolve():
    """Fails on a tree without the feature with SymbolNotShipped."""
    from neuralmonkey_amd.config.builder import resolve_symbol
    from neuralmonkey_amd.readers import image_reader as R
    for name in ("image_reader", "imagenet_reader", "single_image_for_imagenet", "VGG_RGB_MEANS"):
        assert resolve_symbol("readers.image_reader." + name) is getattr(R, name)
        assert resolve_symbol("neuralmonkey.readers.image_reader." + name) is getattr(R, name)
    assert R.VGG_RGB_MEANS == [[[123.68, 116.779, 103.939]]] and R.CHUNK_IMAGES == 64


def test_signatures_are_the_references():
    import inspect
    from neuralmonkey_amd.readers import image_reader as R
    from .test_reference_signatures import product_parameters, read_reference_parameters
    with open(ref.LISTS, encoding="utf-8") as handle:
        lists = json.load(handle)
    assert list(lists) == [PATH] and sorted(lists[PATH]) == ["image_reader", "imagenet_reader"]
    for name in lists[PATH]:
        want = [tuple(p) for p in lists[PATH][name]]
        if os.path.isdir(REF):
            assert read_reference_parameters(PATH, name) == want
        assert product_parameters(PATH, name) == want
    assert [p[0] for p in lists[PATH]["image_reader"]] == ["pad_w", "pad_h", "channels", "prefix", "rescale_w",
                                                            "rescale_h", "keep_aspect_ratio", "mode"]
    defaults = {k: p.default for k, p in inspect.signature(R.image_reader).parameters.items()}
    assert defaults == dict(pad_w=inspect.Parameter.empty, pad_h=inspect.Parameter.empty, channels=3, prefix="",
                            rescale_w=False, rescale_h=False, keep_aspect_ratio=False, mode="RGB")
    defaults = {k: p.default for k, p in inspect.signature(R.imagenet_reader).parameters.items()}
    assert defaults == dict(prefix=inspect.Parameter.empty, target_width=227, target_height=227, vgg_normalization=False,
                            zero_one_normalization=False)
    assert list(inspect.signature(R.single_image_for_imagenet).parameters) == [
        "path", "target_height", "target_width", "vgg_normalization", "zero_one_normalization"]


def reference_text():
    text = open(os.path.join(REF, "neuralmonkey", PATH)).read()
    return re.sub(r"[\"']\s*\n\s*\(?[\"']", "", text)


def test_refusals_use_the_references_words(tmp_path):
    from neuralmonkey_amd.readers.image_reader import image_reader, imagenet_reader
    texts = []
    with pytest.raises(ValueError) as info:
        image_reader(40, 20, keep_aspect_ratio=True)
    texts.append(str(info.value))
    assert texts[-1] == "It does not make sense to keep the aspect ratio while not rescaling the image."
    for kw in (dict(rescale_w=True), dict(rescale_h=True)):
        with pytest.raises(ValueError) as info:
            image_reader(40, 20, **kw)
        assert str(info.value) == "While rescaling only one side, aspect ratio must be kept, was set to false."
    texts.append(str(info.value))
    for mode in ("P", "CMYK", "I", "1", "rgb"):
        with pytest.raises(NotImplementedError, match="mode '{}'".format(mode)):
            image_reader(40, 20, mode=mode)
    with pytest.raises(TypeError):
        image_reader("40", 20)
    with pytest.raises(TypeError):
        imagenet_reader(prefix=3)
    # a missing file: the reader is lazy, nothing is opened before the first item is asked for
    listing = tmp_path / "files.txt"
    listing.write_text("here.pgm\nnot_here.jpg\n")
    (tmp_path / "here.pgm").write_bytes(ref.pnm_bytes(np.zeros((2, 3), np.uint8)))
    missing = os.path.join(str(tmp_path), "not_here.jpg")
    items = image_reader(40, 20, prefix=str(tmp_path))(["/no/such/list"])
    with pytest.raises(FileNotFoundError):
        next(iter(items))
    listing.write_text("not_here.jpg\n")
    with pytest.raises(Exception) as info:
        next(iter(image_reader(40, 20, prefix=str(tmp_path))([str(listing)])))
    assert type(info.value) is Exception and str(info.value) == "Image file '{}' no.1  does not exist.".format(missing)
    with pytest.raises(Exception) as info:
        next(iter(imagenet_reader(str(tmp_path))([str(listing)])))
    assert type(info.value) is Exception and str(info.value) == "Image file '{}' no. 1 does not exist.".format(missing)
    # the declared number of channels against the mode's
    listing.write_text("here.pgm\n")
    for mode, channels, has in (("RGB", 1, 3), ("L", 3, 1), ("F", 3, 1)):
        with pytest.raises(ValueError) as info:
            next(iter(image_reader(40, 20, channels=channels, prefix=str(tmp_path), mode=mode)([str(listing)])))
        assert str(info.value) == "Image does not have the pre-declared number of channels {}, but {}.".format(channels,
                                                                                                              has)
    texts.append("Image does not have the pre-declared number of channels {}, but {}.")
    # a resize to a zero extent: Pillow's ValueError (1 x 50 with the aspect kept -> 0 x 20)
    (tmp_path / "thin.pgm").write_bytes(ref.pnm_bytes(np.zeros((50, 1), np.uint8)))
    listing.write_text("thin.pgm\n")
    reader = image_reader(40, 20, channels=1, prefix=str(tmp_path), rescale_w=True, rescale_h=True,
                          keep_aspect_ratio=True, mode="L")
    with pytest.raises(ValueError, match="height and width must be > 0"):
        next(iter(reader([str(listing)])))
    with pytest.raises(AssertionError):                     # the reference's shape assertion has the two swapped
        next(iter(imagenet_reader(str(tmp_path), target_width=16, target_height=8)([str(listing)])))
    if os.path.isdir(REF):
        text = reference_text().replace("'", "").replace('"', "")
        for message in texts + ["Image file {} no.{}  does not exist.", "Image file {} no. {} does not exist.",
                                "Skipping image from file {} no. {}.", "Image should have either 2 (black and white) or "
                                "three dimensions (color channels), has {} dimension."]:
            assert message.replace("'", "").replace('"', "") in text, message


def test_geometry_follows_the_reference_line_by_line():
    from neuralmonkey_amd.readers.image_reader import BICUBIC, BILINEAR, plan_image

    def plan(w, h, *flags):
        g = plan_image(w, h, 40, 20, *flags)
        return (g.new_w, g.new_h, g.filt, g.crop_x, g.crop_y, g.copy_w, g.copy_h)
    assert plan(40, 20, True, True, False) == (40, 20, None, 0, 0, 40, 20)           # the early return
    assert plan(53, 37, True, True, False) == (40, 20, BILINEAR, 0, 0, 40, 20)
    assert plan(53, 37, True, True, True) == (28, 20, BICUBIC, 0, 0, 28, 20)
    assert plan(3, 50, True, True, True) == (1, 20, BICUBIC, 0, 0, 1, 20)
    assert plan(53, 37, True, False, True) == (40, 27, BICUBIC, 0, 3, 40, 20)        # 7 = 3 + 4: rows 3 .. 23
    assert plan(53, 37, False, True, True) == (28, 20, BICUBIC, 0, 0, 28, 20)
    assert plan(40, 37, True, False, True) == (40, 37, None, 0, 8, 40, 20)           # the width fits: no resize
    assert plan(53, 37, False, False, False) == (53, 37, None, 6, 8, 40, 20)
    assert plan(10, 7, False, False, False) == (10, 7, None, 0, 0, 10, 7)
    assert plan(41, 20, False, False, False) == (41, 20, None, 0, 0, 40, 20)
    with pytest.raises(ValueError):
        plan(1, 50, True, True, True)
    with pytest.raises(ValueError):
        plan(500, 3, True, False, True)


def test_tables_are_pillows():
    from neuralmonkey_amd.readers.image_reader import BICUBIC, BILINEAR, fixed_point, identity_table, resample_table
    up = resample_table(2, 4, BILINEAR)
    assert up.first.tolist() == [0, 0, 0, 1] and up.count.tolist() == [1, 2, 2, 1] and up.k.shape == (4, 3)
    assert np.array_equal(up.k, [[1, 0, 0], [0.75, 0.25, 0], [0.25, 0.75, 0], [1, 0, 0]])
    down = resample_table(700, 256, BILINEAR)
    assert down.k.shape[1] == 2 * 3 + 1 and down.count.max() > 3
    cubic = resample_table(37, 20, BICUBIC)
    assert cubic.k.shape[1] == 2 * 4 + 1 and (cubic.k < 0).any() and np.abs(cubic.k).sum(1).max() < 1.3
    for table, size in ((up, 2), (down, 700), (cubic, 37)):
        assert table.first.dtype == table.count.dtype == np.int32 and table.k.dtype == np.float64
        assert (table.first >= 0).all() and (table.first + table.count <= size).all() and (table.count >= 1).all()
        assert np.abs(table.k.sum(1) - 1).max() < 1e-15
        live = np.arange(table.k.shape[1])[None] < table.count[:, None]
        assert not table.k[~live].any()
    one = identity_table(5)
    assert one.first.tolist() == [0, 1, 2, 3, 4] and (one.count == 1).all() and np.array_equal(one.k, np.ones((5, 1)))
    assert fixed_point(np.array([1.0, 0.5, -0.125, 1e-9, -1e-9])).tolist() == [1 << 22, 1 << 21, -(1 << 19), 0, 0]
    assert fixed_point(np.array([0.3])).dtype == np.int32


# ---- decoding ----------------------------------------------------------------------------------------------------------------
def test_pnm_parser_on_hand_written_bytes():
    from neuralmonkey_amd.readers.image_reader import parse_pnm
    grey = parse_pnm(b"P5\n3 2\n255\n" + bytes([0, 1, 2, 253, 254, 255]))
    assert grey.dtype == np.uint8 and grey.tolist() == [[0, 1, 2], [253, 254, 255]]
    colour = parse_pnm(b"P6 2 1 255 " + bytes([9, 8, 7, 1, 2, 3]))
    assert colour.shape == (1, 2, 3) and colour.tolist() == [[[9, 8, 7], [1, 2, 3]]]
    commented = parse_pnm(b"P5\n# made by hand\n2 # width\n1\n255\n" + bytes([10, 32]))      # 10 and 32 are whitespace bytes
    assert commented.tolist() == [[10, 32]]
    colour[0, 0, 0] = 1                                                   # a writable copy
    for bad in (b"P5\n3 2\n65535\n" + bytes(12), b"P5\n3 2\n255\n" + bytes(5), b"P2\n1 1\n255\n0\n", b"P5\n0 2\n255\n",
                b"P5\nx 2\n255\n", b"\xff\xd8\xff\xe0", b""):
        assert parse_pnm(bad) is None
    for pixels in (np.arange(6, dtype=np.uint8).reshape(2, 3), np.arange(24, dtype=np.uint8).reshape(2, 4, 3)):
        assert np.array_equal(parse_pnm(ref.pnm_bytes(pixels)), pixels)


def test_decode_reads_pnm_without_pillow_and_names_it_when_it_is_missing(tmp_path, monkeypatch):
    from neuralmonkey_amd.readers.image_reader import decode
    pixels = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)
    (tmp_path / "named.jpg").write_bytes(ref.pnm_bytes(pixels))          # the content is sniffed, not the name
    (tmp_path / "garbage.jpg").write_bytes(b"no image at all")
    with pytest.raises(IOError):
        decode(str(tmp_path / "garbage.jpg"))
    for name in [m for m in sys.modules if m == "PIL" or m.startswith("PIL.")]:
        monkeypatch.setitem(sys.modules, name, None)
    monkeypatch.setitem(sys.modules, "PIL", None)
    assert np.array_equal(decode(str(tmp_path / "named.jpg")), pixels)
    with pytest.raises(ImportError, match=r"Pillow \(PIL\), which is not installed"):
        decode(str(tmp_path / "garbage.jpg"))


def test_decode_converts_other_source_modes_on_the_host(tmp_path):
    from PIL import Image
    from neuralmonkey_amd.readers.image_reader import decode
    rng = np.random.default_rng(3)
    rgba = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    Image.fromarray(rgba, "RGBA").save(str(tmp_path / "rgba.png"))
    Image.fromarray(rgba[..., 0]).save(str(tmp_path / "grey.png"))
    Image.fromarray(rgba[..., 0] > 127).save(str(tmp_path / "bits.png"))
    assert np.array_equal(decode(str(tmp_path / "rgba.png")), rgba[..., :3])
    assert np.array_equal(decode(str(tmp_path / "grey.png")), rgba[..., 0])
    assert np.array_equal(decode(str(tmp_path / "bits.png")), np.where(rgba[..., 0] > 127, 255, 0))


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
def test_fixture_holds_the_issues_cases():
    cases, arrays = ref.fixture()
    names = [c["name"] for c in cases]
    assert len(names) == len(set(names)) == 47 and os.path.getsize(ref.FIXTURE) < 1 << 20
    group_a = [c for c in cases if c["name"].startswith("a_")]
    sizes = [ref.source_of(c).shape[1::-1] for c in group_a]
    assert len(group_a) == 10 and sizes[:2] == [(219, 31), (58, 31)]
    assert sizes[4:] == [(1, 1), (2, 3), (256, 32), (256, 31), (300, 32), (700, 90)]
    assert all(c["kwargs"] == dict(pad_w=256, pad_h=32, rescale_w=True, rescale_h=True, mode="F", channels=1)
               for c in group_a)
    for mode in ("L", "RGB"):
        assert sum(1 for n in names if re.match(r"b[1-5]_{}_".format(mode), n)) == 9
    assert sum(1 for n in names if n.startswith("b6_")) == 6 and sum(1 for n in names if n.startswith("d_")) == 12
    for case in cases:
        pixels, want = ref.source_of(case), ref.want_of(case)
        assert pixels.dtype == np.uint8 and pixels.ndim in (2, 3)
        kw = case["kwargs"]
        if case["reader"] == "image_reader":
            assert want.dtype == np.float32 and want.shape == (kw["pad_h"], kw["pad_w"], kw["channels"])
        else:
            assert want.shape == (16, 16, 3)
    colour = arrays["src/rgb_53x37"].astype(int)
    assert np.abs(colour[..., 0] - colour[..., 1]).mean() > 40             # the colour weights are exercised
    assert ref.want_of(next(c for c in cases if c["name"] == "b5_L_10x7"))[7:, :, :].max() == 0


@pytest.mark.parametrize("name", [c["name"] for c in ref.fixture()[0]])
def test_product_tables_and_geometry_reproduce_the_reference_exactly(name):
    case, = [c for c in ref.fixture()[0] if c["name"] == name]
    plan, sub, divide = ref.build_plan([case])
    got = ref.run_plan(plan, sub, divide)
    want = ref.want_of(case)
    assert got.dtype == np.float32 and got.shape == (1,) + want.shape
    assert np.array_equal(got[0], want.astype(np.float32)), (name, np.abs(got[0] - want).max())


def test_a_case_alone_equals_the_case_inside_a_chunk():
    """The plan of a chunk is the plans of its images side by side (CPU part; the kernels: test_image_reader_kernels_gpu)."""
    cases = ref.cases_of(reader="image_reader", mode="RGB", prefix="b")             # all of them 40 x 20
    plan, _, _ = ref.build_plan(cases)
    assert len(cases) == 12
    assert plan.offs.shape == (6, len(cases) + 1) and (np.diff(plan.offs, axis=1) >= 0).all()
    assert plan.offs[4, 0] == plan.offs[2, -1] and plan.offs[4, -1] == len(plan.bounds)
    assert plan.offs[5, -1] == len(plan.coef) and plan.coef.dtype == np.int32 and plan.offs[0, -1] == len(plan.src)
    together = ref.run_plan(plan)
    for i, case in enumerate(cases):
        assert np.array_equal(together[i], ref.want_of(case)), case["name"]


def test_real_jpegs_through_pillow_match_pillows_own_resize(tmp_path):
    """The host part on the reference's 40 JPEGs: decode, plan and tables, applied by the restatement, against the same
    pipeline called on Pillow directly (the decoder is the same build on both sides, so equality is exact)."""
    from PIL import Image
    from neuralmonkey_amd.readers.image_reader import ChunkPlan, decode, plan_image
    with tarfile.open(ref.ARCHIVE) as tar:
        names = sorted(m.name for m in tar.getmembers())
        tar.extractall(str(tmp_path))
    assert len(names) == 40 and all(n.startswith("tests/data/str/") and n.endswith(".jpg") for n in names)
    assert os.path.getsize(ref.ARCHIVE) < 1 << 20
    if os.path.isdir(REF):
        for rel in names:
            with open(os.path.join(REF, rel), "rb") as a, open(os.path.join(str(tmp_path), rel), "rb") as b:
                assert a.read() == b.read(), rel
    images = [decode(os.path.join(str(tmp_path), n)) for n in names]
    plan = ChunkPlan(images, [plan_image(p.shape[1], p.shape[0], 256, 32, True, True, False) for p in images], "F", 256,
                     32)
    got = ref.run_plan(plan)
    for i, name in enumerate(names):
        want = np.array(Image.open(os.path.join(str(tmp_path), name)).convert("F").resize((256, 32), Image.BILINEAR))
        assert np.array_equal(got[i, :, :, 0], want), name


# ---- the binding table -------------------------------------------------------------------------------------------------------
def imgread_header_symbols():
    text = open(os.path.join(ROOT, "include", "nmhip_imgread.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nm_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


def test_imgread_header_matches_its_binding_table(lib):
    from neuralmonkey_amd import _lib
    from .test_abi import header_symbols
    mine = imgread_header_symbols()
    assert mine == set(_lib.IMGREAD_SIGNATURES) == {"nm_imgread_rows", "nm_imgread_cols", "nm_imgread_check"}
    assert not mine & header_symbols() and not mine & set(_lib.SIGNATURES)
    for name, (res, args) in _lib.IMGREAD_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_chunk_check_refuses_a_plan_that_does_not_fit(lib):
    """nm_imgread_check reads host arrays only: it runs without a GPU."""
    from neuralmonkey_amd import _lib, ops
    plan, _, _ = ref.build_plan(ref.cases_of(prefix="b5_L"))
    ops.imgread_check(plan.offs, plan.geom, plan.target, plan.pad_w, plan.pad_h)
    for edit, text in ((lambda o, g: g.__setitem__((1, 2), 2), "image 1 has 2 bands"),
                       (lambda o, g: g.__setitem__((0, 7), 41), "image 0 copies 41 x 20 into 40 x 20"),
                       (lambda o, g: g.__setitem__((2, 0), -1), "image 2 has a negative geometry field 0"),
                       (lambda o, g: g.__setitem__((0, 10), 30), "image 0 reads rows 8 + 30 of 37"),
                       (lambda o, g: o.__setitem__((0, 1), o[0, 1] - 1), "image 0 needs 5883 entries of array 0"),     # 53 * 37 * 3
                       (lambda o, g: o.__setitem__((1, 2), o[1, 1] - 1), "image 1 needs 70 entries of array 1"),
                       (lambda o, g: o.__setitem__((5, 3), o[5, 3] - 1), "image 2 needs 20 entries of array 5")):
        offs, geom = plan.offs.copy(), plan.geom.copy()
        edit(offs, geom)
        with pytest.raises(_lib.NMHipError, match=re.escape(text)):
            ops.imgread_check(offs, geom, plan.target, plan.pad_w, plan.pad_h)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert lib.nm_imgread_check(None, None, 1, 0, 1, 1) < 0 and b"null pointer" in lib.nm_last_error()


def test_kernels_of_the_reader_do_not_spill(lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_resources
    finally:
        sys.path.pop(0)
    mine = {k: v for k, v in kernel_resources().items() if "imgread_rows_kernel" in k or "imgread_cols_kernel" in k}
    assert len(mine) == 4, sorted(mine)
    assert all(v["scratch"] == 0 for v in mine.values()), {k: v["scratch"] for k, v in mine.items()}
