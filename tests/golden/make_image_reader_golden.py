"""The fixtures of the image reader's tests, made where the reference tree and Pillow are:

    python tests/golden/make_image_reader_golden.py

* tests/golden/image_reader_golden.npz -- for every case the decoded source pixels (``src/<source>``, uint8), the
  configuration (``cases``, JSON) and the array the reference's readers/image_reader.py yields (``out/<case>``).  The
  reference module is imported from its file unmodified and run with this machine's Pillow on files written to a
  temporary directory (PNG, lossless; the JPEG cases read the reference's own files).  Outputs whose values are all
  exact in float32 are stored as float32, the others (imagenet_reader's normalised arrays) as float64;
* tests/golden/reference_tests_str_images.tar.gz -- the 40 JPEGs of the reference's tests/data/str, its bytes;
* tests/golden/image_reader_signatures.json -- the two readers' parameters, read from the reference's source as
  tests/test_reference_signatures.py reads them.

Data only: no program text of the reference is written anywhere."""
import glob
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_reference_ini_fixture import REF, members, write  # noqa: E402  pylint: disable=wrong-import-position

OUT = os.path.join(HERE, "image_reader_golden.npz")
OUT_IMAGES = os.path.join(HERE, "reference_tests_str_images.tar.gz")
OUT_SIGNATURES = os.path.join(HERE, "image_reader_signatures.json")
SIGNATURES = [("readers/image_reader.py", "image_reader"), ("readers/image_reader.py", "imagenet_reader")]
STR = dict(pad_w=256, pad_h=32, rescale_w=True, rescale_h=True, mode="F", channels=1)
JPEG_SIZES = [(219, 31), (58, 31)]               # two of the four JPEG cases are picked by their size
SYNTHETIC = [(1, 1), (2, 3), (256, 32), (256, 31), (300, 32), (700, 90), (53, 37), (200, 20), (3, 50), (10, 7), (41, 20),
             (16, 16)]


def reference_module():
    """readers/image_reader.py of the reference, imported from its file; the two modules it imports that are not
    installed here (typeguard, neuralmonkey.logging) are stand-ins that check nothing and warn through ``warnings``."""
    import warnings
    typeguard = types.ModuleType("typeguard")
    typeguard.check_argument_types = lambda: True
    package, logging = types.ModuleType("neuralmonkey"), types.ModuleType("neuralmonkey.logging")
    logging.warn = warnings.warn
    package.logging = logging
    sys.modules.update({"typeguard": typeguard, "neuralmonkey": package, "neuralmonkey.logging": logging})
    spec = importlib.util.spec_from_file_location("reference_image_reader",
                                                  os.path.join(REF, "neuralmonkey/readers/image_reader.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def sources():
    """name -> (pixels, path of a file that decodes to exactly them)."""
    from PIL import Image
    found = {}
    paths = sorted(glob.glob(os.path.join(REF, "tests/data/str/*.jpg")))
    sizes = {p: Image.open(p).size for p in paths}
    picked = [next(p for p in paths if sizes[p] == size) for size in JPEG_SIZES]
    picked += [p for p in paths if p not in picked][:2]
    for path in picked:
        pixels = np.array(Image.open(path))
        assert pixels.dtype == np.uint8 and Image.open(path).mode in ("L", "RGB")
        found["jpeg_{}x{}_{}".format(pixels.shape[1], pixels.shape[0], os.path.basename(path)[:-4])] = (pixels, path)
    rng = np.random.default_rng(20261020)
    tmp = tempfile.mkdtemp(prefix="image_reader_golden")
    for w, h in SYNTHETIC:
        for kind, shape in (("rgb", (h, w, 3)), ("l", (h, w))):
            if kind == "l" and (w, h) != (53, 37):
                continue
            pixels = rng.integers(0, 256, shape, dtype=np.uint8)           # R, G and B independent
            name = "{}_{}x{}".format(kind, w, h)
            path = os.path.join(tmp, name + ".png")
            Image.fromarray(pixels).save(path)
            assert np.array_equal(np.array(Image.open(path)), pixels)
            found[name] = (pixels, path)
    return found


def cases(found):
    """[(case name, reader, source, kwargs)]: the groups a-d of the tests' module docstrings."""
    out = []
    for name in found:
        if name.startswith("jpeg_"):
            out.append(("a_" + name, "image_reader", name, STR))
    for w, h in SYNTHETIC[:6]:
        out.append(("a_rgb_{}x{}".format(w, h), "image_reader", "rgb_{}x{}".format(w, h), STR))
    for mode, channels in (("L", 1), ("RGB", 3)):
        base = dict(pad_w=40, pad_h=20, mode=mode, channels=channels)
        both = dict(base, rescale_w=True, rescale_h=True)
        out.append(("b1_{}_53x37".format(mode), "image_reader", "rgb_53x37", both))
        for size in ("53x37", "200x20", "3x50"):
            out.append(("b2_{}_{}".format(mode, size), "image_reader", "rgb_" + size, dict(both, keep_aspect_ratio=True)))
        out.append(("b3_{}_53x37".format(mode), "image_reader", "rgb_53x37",
                    dict(base, rescale_w=True, keep_aspect_ratio=True)))
        out.append(("b4_{}_53x37".format(mode), "image_reader", "rgb_53x37",
                    dict(base, rescale_h=True, keep_aspect_ratio=True)))
        for size in ("53x37", "10x7", "41x20"):
            out.append(("b5_{}_{}".format(mode, size), "image_reader", "rgb_" + size, base))
    for label, extra in (("bilinear", dict(rescale_w=True, rescale_h=True)),
                         ("bicubic", dict(rescale_w=True, rescale_h=True, keep_aspect_ratio=True)), ("crop", {})):
        out.append(("b6_l_to_rgb_" + label, "image_reader", "l_53x37",
                    dict(pad_w=40, pad_h=20, mode="RGB", channels=3, **extra)))
        out.append(("b6_rgb_to_f_" + label, "image_reader", "rgb_53x37",
                    dict(pad_w=40, pad_h=20, mode="F", channels=1, **extra)))
    out.append(("c_rgb_53x37", "image_reader", "rgb_53x37",
                dict(pad_w=300, pad_h=5, mode="RGB", channels=3, rescale_w=True, rescale_h=True)))
    for size in ("53x37", "10x7", "16x16"):
        for vgg in (False, True):
            for unit in (False, True):
                out.append(("d_{}_vgg{}_unit{}".format(size, int(vgg), int(unit)), "imagenet_reader", "rgb_" + size,
                            dict(target_width=16, target_height=16, vgg_normalization=vgg, zero_one_normalization=unit)))
    return out


def main():
    reference = reference_module()
    found = sources()
    arrays = {"src/" + name: pixels for name, (pixels, _) in found.items()}
    listed = []
    tmp = tempfile.mkdtemp(prefix="image_reader_lists")
    for case, reader, source, kwargs in cases(found):
        list_file = os.path.join(tmp, case + ".txt")
        with open(list_file, "w") as handle:
            handle.write(found[source][1] + "\n")
        got, = list(getattr(reference, reader)(prefix="", **kwargs)([list_file]))
        assert got.dtype == np.float64
        arrays["out/" + case] = got.astype(np.float32) if np.array_equal(got.astype(np.float32), got) else got
        listed.append(dict(name=case, reader=reader, source=source, kwargs=kwargs))
    arrays["cases"] = np.array(json.dumps(listed))
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), len(listed), "cases")
    assert os.path.getsize(OUT) < 1 << 20
    write(OUT_IMAGES, members([], ["str/*.jpg"]))
    assert os.path.getsize(OUT_IMAGES) < 1 << 20
    from tests.test_reference_signatures import read_reference_parameters
    lists = {}
    for path, name in SIGNATURES:
        lists.setdefault(path, {})[name] = read_reference_parameters(path, name)
    with open(OUT_SIGNATURES, "w", encoding="utf-8") as handle:
        json.dump(lists, handle, indent=1)
        handle.write("\n")
    print(OUT_SIGNATURES)


if __name__ == "__main__":
    main()
