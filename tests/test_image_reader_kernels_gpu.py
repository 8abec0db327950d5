"""The two kernels of csrc/nm_imgread.hip on the MI355X, through ``readers.image_reader.ChunkPlan`` -> ops -> the C ABI,
on the decoded pixels of tests/golden/image_reader_golden.npz (its cases: tests/test_image_reader_host.py) against the
arrays the reference's reader produced with Pillow.

Tolerances.  The modes L and RGB are integer arithmetic: equality, no tolerance.  imagenet_reader's arrays are one
float64 subtraction and division of exact integers rounded once: equality with ``np.float32(recorded)``.  Mode F is
expected to be equal too (float64 sums in Pillow's tap order, one rounding to float32 per pass); the assertion is
``max |got - want| <= 2^-15``, one float32 ulp for magnitudes in [256, 512) -- bicubic overshoot of 0..255 data stays
below 512 because the sum of |k| is below 1.3 -- and the number of elements that differ at all is printed (DESIGN 4.19
records it)."""
import ctypes
import os
import warnings

import numpy as np
import pytest

from . import image_reader_ref as ref

pytestmark = pytest.mark.gpu

_ALONE = {}


def alone(case):
    """The case as a chunk of one image, computed once."""
    if case["name"] not in _ALONE:
        plan, sub, divide = ref.build_plan([case])
        got = plan.run(sub, divide)
        assert got.dtype == np.float32 and got.shape[0] == 1
        got.setflags(write=False)
        _ALONE[case["name"]] = got[0]
    return _ALONE[case["name"]]


def chunks():
    """The fixture's cases grouped into chunks that share a target, a size and an epilogue."""
    groups = {}
    for case in ref.fixture()[0]:
        kw = case["kwargs"]
        key = (case["reader"], kw.get("mode"), kw.get("pad_w"), kw.get("pad_h"), kw.get("vgg_normalization"),
               kw.get("zero_one_normalization"))
        groups.setdefault(key, []).append(case)
    return list(groups.values())


@pytest.mark.parametrize("mode", ["L", "RGB"])
def test_8bit_modes_equal_pillow_byte_for_byte(dev, mode):
    cases = ref.cases_of(reader="image_reader", mode=mode)
    assert len(cases) == {"L": 9, "RGB": 13}[mode]
    for case in cases:
        got, want = alone(case), ref.want_of(case)
        assert got.shape == want.shape, case["name"]
        differing = int((got != want).sum())
        print("imgread {:<28} {} of {} elements differ".format(case["name"], differing, want.size))
        assert np.array_equal(got, want), case["name"]


def test_imagenet_reader_cases_equal_the_rounded_reference(dev):
    cases = ref.cases_of(reader="imagenet_reader")
    assert len(cases) == 12
    for case in cases:
        got, want = alone(case), ref.want_of(case).astype(np.float32)
        assert np.array_equal(got, want), (case["name"], np.abs(got - want).max())
    plain = alone(next(c for c in cases if c["name"] == "d_10x7_vgg0_unit0"))
    assert not plain[7:].any() and not plain[:, 10:].any() and plain[:7, :10].any()
    shifted = alone(next(c for c in cases if c["name"] == "d_10x7_vgg1_unit0"))     # the means leave the padding too
    assert np.array_equal(shifted[15, 15], -np.array([123.68, 116.779, 103.939]).astype(np.float32))


def test_mode_f_is_within_one_ulp_of_pillow(dev):
    cases = ref.cases_of(reader="image_reader", mode="F")
    assert len(cases) == 13
    differing = total = 0
    worst = 0.0
    for case in cases:
        got, want = alone(case), ref.want_of(case)
        assert got.shape == want.shape and np.isfinite(got).all(), case["name"]
        err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        differing += int((got != want).sum())
        total += want.size
        worst = max(worst, err)
        print("imgread {:<40} max |got - want| {:.3e}, {} of {} elements differ".format(
            case["name"], err, int((got != want).sum()), want.size))
    print("imgread mode F: {} of {} elements differ at all, worst {:.3e}".format(differing, total, worst))
    assert worst <= 2.0 ** -15


def test_a_case_alone_equals_the_case_inside_a_chunk_bit_for_bit(dev):
    groups = chunks()
    assert sum(len(g) for g in groups) == 47 and max(len(g) for g in groups) >= 10
    for group in groups:
        plan, sub, divide = ref.build_plan(group)
        together = plan.run(sub, divide)
        again = plan.run(sub, divide)
        assert together.tobytes() == again.tobytes()                                  # no atomics: two runs are equal
        for i, case in enumerate(group):
            assert together[i].tobytes() == alone(case).tobytes(), case["name"]


def test_padding_is_written_as_zeros_over_a_poisoned_buffer(dev):
    import torch
    for name in ("b5_L_10x7", "b4_RGB_53x37", "b2_L_3x50", "b5_RGB_10x7"):
        case, = [c for c in ref.fixture()[0] if c["name"] == name]
        plan, _, _ = ref.build_plan([case])
        out = torch.full((1, plan.pad_h, plan.pad_w, plan.channels), float("nan"), device=dev)
        got = plan.run(out=out)[0]
        ch, cw = int(plan.geom[0, 8]), int(plan.geom[0, 7])
        assert (ch, cw) != (plan.pad_h, plan.pad_w)
        assert got[ch:].tobytes() == bytes(got[ch:].nbytes) and got[:, cw:].tobytes() == bytes(got[:, cw:].nbytes), name
        assert np.array_equal(got, ref.want_of(case)), name


def write_tree(root, cases):
    names = []
    for i, case in enumerate(cases):
        names.append("{:02d}.jpg".format(i))                       # the content is sniffed, as Pillow does
        with open(os.path.join(root, names[-1]), "wb") as handle:
            handle.write(ref.pnm_bytes(ref.source_of(case)))
    names.insert(5, "broken.jpg")
    with open(os.path.join(root, "broken.jpg"), "wb") as handle:
        handle.write(b"no image at all: nothing Pillow reads")
    with open(os.path.join(root, "files.txt"), "w") as handle:
        handle.write("\n".join(names) + "\n")
    return os.path.join(root, "files.txt")


def test_reader_yields_the_same_arrays_in_the_same_order_for_any_chunk_size(dev, tmp_path, monkeypatch):
    from neuralmonkey_amd.readers import image_reader as R
    cases = ref.cases_of(prefix="a_")
    listing = write_tree(str(tmp_path), cases)
    try:
        import PIL  # noqa: F401  pylint: disable=unused-import
    except ImportError:                                 # without Pillow the broken file is an ImportError: leave it out
        lines = [n for n in open(listing).read().split() if n != "broken.jpg"]
        with open(listing, "w") as handle:
            handle.write("\n".join(lines) + "\n")
    broken = "broken.jpg" in open(listing).read()
    reader = R.image_reader(256, 32, channels=1, prefix=str(tmp_path), rescale_w=True, rescale_h=True, mode="F")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        whole = list(reader([listing]))
        monkeypatch.setattr(R, "CHUNK_IMAGES", 3)
        items = reader([listing])
        first = next(items)                                      # lazy: a generator, one array per line
        small = [first] + list(items)
        monkeypatch.setattr(R, "CHUNK_PIXELS", 1)
        single = list(reader([listing, listing]))
    assert len(whole) == len(small) == len(cases) + broken and len(single) == 2 * len(whole)
    want = [ref.want_of(c) for c in cases]
    if broken:
        want.insert(5, np.zeros((32, 256, 1), np.float32))
        texts = [str(w.message) for w in caught]
        assert texts.count("Skipping image from file '{}' no. '6'.".format(os.path.join(str(tmp_path), "broken.jpg"))) == 4
    for i, array in enumerate(want):
        assert whole[i].dtype == np.float32 and whole[i].shape == (32, 256, 1)
        assert whole[i].tobytes() == small[i].tobytes() == single[i].tobytes() == single[len(want) + i].tobytes(), i
        assert np.abs(whole[i] - array).max() <= 2.0 ** -15, i
    # a missing file is reported after the images before it have been yielded
    with open(listing, "w") as handle:
        handle.write("00.jpg\n01.jpg\nnot_here.jpg\n02.jpg\n")
    items = reader([listing])
    assert next(items).tobytes() == whole[0].tobytes() and next(items).tobytes() == whole[1].tobytes()
    with pytest.raises(Exception, match="no.3  does not exist"):
        next(items)
    one = R.single_image_for_imagenet(os.path.join(str(tmp_path), "00.jpg"), 16, 16, True, True)
    assert one.shape == (16, 16, 3) and one.dtype == np.float32


def test_every_refusal_returns_its_text_and_launches_nothing(dev):
    """Host buffers and a null stream: a call that got as far as a launch would fault or fail differently."""
    from neuralmonkey_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    ints = (ctypes.c_int32 * 4096)()
    longs = (ctypes.c_int64 * 64)()
    sub = (ctypes.c_double * 3)()

    def check(fn, cases):
        for kwargs, text in cases:
            assert fn(**kwargs) < 0 and lib.nm_last_error().startswith(text), (kwargs, lib.nm_last_error())

    def rows(src=buf, nbytes=100, offs=longs, geom=ints, n=2, bounds=ints, nb=10, coef=ints, nk=10, target=0, pad_w=40,
             max_rows=8, scratch=buf, ns=100):
        return lib.nm_imgread_rows(None, src, nbytes, offs, geom, n, bounds, nb, coef, nk, target, pad_w, max_rows, scratch,
                                   ns)
    null = b"nm_imgread_rows: null pointer"
    check(rows, [(dict(src=None), null), (dict(offs=None), null), (dict(geom=None), null), (dict(bounds=None), null),
                 (dict(coef=None), null), (dict(scratch=None), null),
                 (dict(n=0), b"nm_imgread_rows: N = 0 images outside 1..65535"),
                 (dict(n=65536), b"nm_imgread_rows: N = 65536 images outside 1..65535"),
                 (dict(target=3), b"nm_imgread_rows: unknown target 3"),
                 (dict(target=-1), b"nm_imgread_rows: unknown target -1"),
                 (dict(pad_w=0), b"nm_imgread_rows: pad_w 0 outside"),
                 (dict(max_rows=-1), b"nm_imgread_rows: max_rows -1 outside"),
                 (dict(max_rows=8 * 65535 + 1), b"nm_imgread_rows: max_rows 524281 beyond one grid"),
                 (dict(nbytes=-1), b"nm_imgread_rows: negative size"), (dict(ns=-1), b"nm_imgread_rows: negative size"),
                 (dict(nb=-1), b"nm_imgread_rows: negative size"), (dict(nk=-1), b"nm_imgread_rows: negative size")])
    assert rows(max_rows=0, src=None, scratch=None) == 0 and rows(nbytes=0, src=None) == 0           # no-ops

    def cols(scratch=buf, ns=100, offs=longs, geom=ints, n=2, bounds=ints, nb=10, coef=ints, nk=10, target=1, pad_w=40,
             pad_h=20, means=sub, divide=255.0, out=buf, ld=120):
        return lib.nm_imgread_cols(None, scratch, ns, offs, geom, n, bounds, nb, coef, nk, target, pad_w, pad_h, means,
                                   divide, out, ld)
    null = b"nm_imgread_cols: null pointer"
    check(cols, [(dict(scratch=None), null), (dict(offs=None), null), (dict(geom=None), null), (dict(bounds=None), null),
                 (dict(coef=None), null), (dict(out=None), null),
                 (dict(n=0), b"nm_imgread_cols: N = 0 images outside 1..65535"),
                 (dict(target=3), b"nm_imgread_cols: unknown target 3"),
                 (dict(pad_w=0), b"nm_imgread_cols: pad_w 0, pad_h 20 outside"),
                 (dict(pad_h=0), b"nm_imgread_cols: pad_w 40, pad_h 0 outside"),
                 (dict(ld=119), b"nm_imgread_cols: ld 119 below pad_w * C = 120"),
                 (dict(target=2, ld=39), b"nm_imgread_cols: ld 39 below pad_w * C = 40"),
                 (dict(n=65535, pad_h=1 << 10, ld=1 << 10), b"nm_imgread_cols: N * pad_h * ld = 65535 * 1024 * 1024"),
                 (dict(pad_h=1 << 30), b"nm_imgread_cols: N * pad_h * ld = 2 * 1073741824 * 120"),
                 (dict(divide=0.0), b"nm_imgread_cols: divide 0"),
                 (dict(ns=-1), b"nm_imgread_cols: negative size"), (dict(nb=-1), b"nm_imgread_cols: negative size"),
                 (dict(nk=-1), b"nm_imgread_cols: negative size")])
    geom = (ctypes.c_int32 * 16)(5, 5, 2, 5, 5, 0, 0, 5, 5, 0, 5, 1, 1)
    assert lib.nm_imgread_check(longs, geom, 1, 0, 40, 20) < 0
    assert lib.nm_last_error() == b"nm_imgread_check: image 0 has 2 bands (1 or 3)"
    assert lib.nm_imgread_check(longs, geom, 1, 5, 40, 20) < 0 and lib.nm_last_error().startswith(b"nm_imgread_check: unknown")
