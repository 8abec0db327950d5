"""NumPy restatement of the two passes of csrc/nm_imgread.hip, and the loader of tests/golden/image_reader_golden.npz.

``run_plan`` applies the PRODUCT's arrays -- the offsets, geometry, bounds and coefficients of a
``readers.image_reader.ChunkPlan``, exactly what is uploaded -- with Pillow's arithmetic: it holds no second copy of the
table or geometry formulas, so comparing its result with the reference's recorded output pins the product's planning on
a machine without a GPU, and comparing the kernels with the same recorded output pins the device arithmetic."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "image_reader_golden.npz")
ARCHIVE = os.path.join(GOLDEN, "reference_tests_str_images.tar.gz")
LISTS = os.path.join(GOLDEN, "image_reader_signatures.json")

_CACHE = {}


def fixture():
    """(cases, arrays): ``cases`` the list of dicts name / reader / source / kwargs; loaded once, never modified."""
    if not _CACHE:
        with np.load(FIXTURE) as z:
            arrays = {k: z[k] for k in z.files}
        for value in arrays.values():
            value.setflags(write=False)
        _CACHE["cases"] = json.loads(str(arrays.pop("cases")))
        _CACHE["arrays"] = arrays
    return _CACHE["cases"], _CACHE["arrays"]


def source_of(case):
    return fixture()[1]["src/" + case["source"]]


def want_of(case):
    return fixture()[1]["out/" + case["name"]]


def cases_of(reader=None, mode=None, prefix=None):
    out = []
    for case in fixture()[0]:
        if reader is not None and case["reader"] != reader:
            continue
        if mode is not None and case["kwargs"].get("mode", "RGB") != mode:
            continue
        if prefix is not None and not case["name"].startswith(prefix):
            continue
        out.append(case)
    return out


def build_plan(cases):
    """The product's ChunkPlan for fixture cases that share a reader configuration's target: -> (plan, sub, divide)."""
    from neuralmonkey_amd.readers import image_reader as R
    images, geometries, seen = [], [], []
    first = cases[0]
    for case in cases:
        pixels, kw = source_of(case), case["kwargs"]
        if case["reader"] == "imagenet_reader":
            mode, pad_w, pad_h = "RGB", kw["target_width"], kw["target_height"]
            geometry = R.plan_image(pixels.shape[1], pixels.shape[0], pad_w, pad_h, False, False, False)
        else:
            mode, pad_w, pad_h = kw["mode"], kw["pad_w"], kw["pad_h"]
            geometry = R.plan_image(pixels.shape[1], pixels.shape[0], pad_w, pad_h, kw.get("rescale_w", False),
                                    kw.get("rescale_h", False), kw.get("keep_aspect_ratio", False))
        images.append(pixels)
        geometries.append(geometry)
        assert len({(mode, pad_w, pad_h)} | set(seen)) == 1, "the cases of one chunk share a target"
        seen.append((mode, pad_w, pad_h))
    kw = first["kwargs"]
    sub, divide = None, 1.0
    if first["reader"] == "imagenet_reader":
        sub = np.array(R.VGG_RGB_MEANS, np.float64).reshape(3) if kw["vgg_normalization"] else None
        divide = 255.0 if kw["zero_one_normalization"] else 1.0
    return R.ChunkPlan(images, geometries, mode, pad_w, pad_h), sub, divide


def convert(pixels, bands, target):
    """Pillow's Image.convert from 8-bit L / RGB to the target mode: [h, w, C] int64 (L, RGB) or float32 (F)."""
    p = pixels.astype(np.int64)
    if target == 1:
        return p if bands == 3 else np.repeat(p, 3, axis=2)
    if bands == 1:
        return p if target == 0 else p.astype(np.float32)
    r, g, b = p[..., 0:1], p[..., 1:2], p[..., 2:3]
    if target == 0:
        return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16
    return (299 * r + 587 * g + 114 * b).astype(np.float32) / np.float32(1000.0)


def one_pass(image, first, count, k, target):
    """Along axis 0 of ``image`` [n_in, ...]: output o = sum over t < count[o] of image[first[o] + t] * k[o, t], taps in
    order; 8-bit: int coefficients, accumulator from 2^21, >> 22, clipped; F: float64 sums, rounded to float32."""
    out = np.zeros((len(first),) + image.shape[1:], np.float32 if target == 2 else np.int64)
    for o in range(len(first)):
        if target == 2:
            acc = np.zeros(image.shape[1:], np.float64)
            for t in range(count[o]):
                acc = acc + image[first[o] + t].astype(np.float64) * k[o, t]
            out[o] = acc.astype(np.float32)
        else:
            acc = np.full(image.shape[1:], 1 << 21, np.int64)
            for t in range(count[o]):
                acc = acc + image[first[o] + t] * int(k[o, t])
            out[o] = np.clip(acc >> 22, 0, 255)
    return out


def run_plan(plan, sub=None, divide=1.0):
    """What the two kernels compute from ``plan``'s arrays: float32 [N, pad_h, pad_w, C]."""
    n, target, channels = len(plan.geom), plan.target, plan.channels
    out = np.zeros((n, plan.pad_h, plan.pad_w, channels), np.float64)
    for i in range(n):
        sw, sh, bands, _, _, _, _, cw, ch, row0, rows, ksh, ksv = (int(v) for v in plan.geom[i, :13])
        pixels = plan.src[plan.offs[0, i]:plan.offs[0, i + 1]].reshape(sh, sw, bands)
        image = convert(pixels, bands, target)[row0:row0 + rows]
        hb = plan.bounds[plan.offs[2, i]:plan.offs[2, i] + cw]
        hk = plan.coef[plan.offs[3, i]:plan.offs[3, i] + cw * ksh].reshape(cw, ksh)
        vb = plan.bounds[plan.offs[4, i]:plan.offs[4, i] + ch]
        vk = plan.coef[plan.offs[5, i]:plan.offs[5, i] + ch * ksv].reshape(ch, ksv)
        across = one_pass(np.swapaxes(image, 0, 1), hb[:, 0], hb[:, 1], hk, target)        # [cw, rows, C]
        assert across.size == plan.offs[1, i + 1] - plan.offs[1, i]
        down = one_pass(np.swapaxes(across, 0, 1), vb[:, 0] - row0, vb[:, 1], vk, target)   # [ch, cw, C]
        out[i, :ch, :cw] = down
    if sub is not None:
        out = out - np.asarray(sub, np.float64).reshape(1, 1, 1, -1)
    if divide != 1.0:
        out = out / divide
    return out.astype(np.float32)


def pnm_bytes(pixels):
    """A decoded image as binary PGM (one band) or PPM (three) bytes."""
    magic = b"P5" if pixels.ndim == 2 else b"P6"
    return magic + "\n{} {}\n255\n".format(pixels.shape[1], pixels.shape[0]).encode() + pixels.tobytes()
