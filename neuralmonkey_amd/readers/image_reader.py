"""Series readers for image files (interface of neuralmonkey/readers/image_reader.py): ``image_reader`` and
``imagenet_reader`` build a reader that takes list files -- one image path per line, relative to ``prefix`` -- and yields
one ``[pad_h, pad_w, channels]`` array per line, in order.

Files are decoded on the host (``PIL.Image.open``; binary PGM / PPM files are parsed here, without Pillow).  Everything
after the decode -- the conversion to the target mode, Pillow's two-pass resize, the centre crop, the zero padding and
the ImageNet normalisation -- runs on the device in two launches per chunk of up to ``CHUNK_IMAGES`` images
(csrc/nm_imgread.hip, include/nmhip_imgread.h), with Pillow's arithmetic: the 8-bit modes byte for byte, mode ``F`` in
float64 sums rounded to float32 once per pass.  The host makes the tables only (``resample_table``, Pillow's
``precompute_coeffs`` in float64) and plans the geometry (``plan_image``, the reference's ``_rescale_or_crop``, ``_crop``
and ``_pad`` line by line).  The arrays are float32 (the reference's are float64; every value is exact in float32)."""
import functools
import os
from typing import Callable, Iterable, Iterator, List, NamedTuple, Optional, Tuple

import numpy as np

from ..checking import check_argument_types

CHUNK_IMAGES = 64                 # images per device chunk ...
CHUNK_PIXELS = 1 << 24            # ... or this many source pixels, whichever fills first

BILINEAR, BICUBIC = 2, 3          # PIL.Image.BILINEAR, PIL.Image.BICUBIC
DEVICE_MODES = {"L": 0, "RGB": 1, "F": 2}          # NM_IMGREAD_L / _RGB / _F
MODE_CHANNELS = {"L": 1, "RGB": 3, "F": 1}
PRECISION_BITS = 22

# the per-channel means (R, G, B) that VGG's preprocessing subtracts
VGG_RGB_MEANS = [[[123.68, 116.779, 103.939]]]


def warn(message: str) -> None:
    """neuralmonkey.logging.warn."""
    import warnings
    warnings.warn(message)


# ---- tables: Pillow's precompute_coeffs -----------------------------------------------------------------------------------
def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    inner = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    outer = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, inner, np.where(x < 2.0, outer, 0.0))


FILTERS = {BILINEAR: (_bilinear, 1.0), BICUBIC: (_bicubic, 2.0)}


class Table(NamedTuple):
    """One axis of a resize: output ``i`` is ``sum_t in[first[i] + t] * k[i, t]`` over ``t < count[i]``."""
    first: np.ndarray       # int32 [out]
    count: np.ndarray       # int32 [out]
    k: np.ndarray           # float64 [out, ksize], zero past count

    def keep(self, start: int, size: int) -> "Table":
        return Table(self.first[start:start + size], self.count[start:start + size], self.k[start:start + size])


def _frozen(*arrays: np.ndarray) -> Table:
    for array in arrays:
        array.setflags(write=False)                  # the tables are cached and shared
    return Table(*arrays)


@functools.lru_cache(maxsize=1024)
def identity_table(size: int) -> Table:
    """The one-tap table of a pass Pillow skips: it copies, in both arithmetic paths."""
    return _frozen(np.arange(size, dtype=np.int32), np.ones(size, np.int32), np.ones((size, 1)))


@functools.lru_cache(maxsize=1024)
def resample_table(in_size: int, out_size: int, filt: int) -> Table:
    """Pillow's coefficients of one axis (src/libImaging/Resample.c:precompute_coeffs), in float64, the weights of an
    output summed in tap order (``cumsum`` is sequential; ``sum`` is pairwise and rounds differently).  Cached: the
    images of a dataset share a few sizes."""
    kernel, filter_support = FILTERS[filt]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = filter_support * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(out_size) + 0.5) * scale
    inv = 1.0 / filterscale
    first = np.maximum(np.trunc(center - support + 0.5), 0.0)
    last = np.minimum(np.trunc(center + support + 0.5), float(in_size))
    count = (last - first).astype(np.int64)
    taps = np.arange(ksize)[None, :]
    live = taps < count[:, None]
    w = np.where(live, kernel((taps + first[:, None] - center[:, None] + 0.5) * inv), 0.0)
    total = np.cumsum(w, axis=1)[:, -1:]
    k = np.where(total != 0.0, w / np.where(total != 0.0, total, 1.0), w)
    return _frozen(first.astype(np.int32), count.astype(np.int32), np.where(live, k, 0.0))


def fixed_point(k: np.ndarray) -> np.ndarray:
    """The 8-bit path's coefficients: ``trunc(+-0.5 + k * 2^22)`` as int32 (Resample.c:normalize_coeffs_8bpc)."""
    scaled = k * float(1 << PRECISION_BITS)
    return np.where(k < 0, np.trunc(-0.5 + scaled), np.trunc(0.5 + scaled)).astype(np.int32)


# ---- geometry: the reference's _rescale_or_crop, _crop and _pad ------------------------------------------------------------
class Geometry(NamedTuple):
    src_w: int
    src_h: int
    new_w: int              # size after the resize (the source's where there is none)
    new_h: int
    filt: Optional[int]     # BILINEAR, BICUBIC or None: no resize
    crop_x: int
    crop_y: int
    copy_w: int
    copy_h: int


def plan_image(src_w: int, src_h: int, pad_w: int, pad_h: int, rescale_w: bool, rescale_h: bool,
               keep_aspect_ratio: bool) -> Geometry:
    """Where the pixels of a ``src_w`` x ``src_h`` image go (readers/image_reader.py:180-226 of the reference)."""
    new_w, new_h, filt = src_w, src_h, None
    if not (src_w == pad_w and src_h == pad_h):              # (the early return: nothing is resized or cropped)
        if rescale_w and rescale_h and not keep_aspect_ratio:
            new_w, new_h, filt = pad_w, pad_h, BILINEAR
        elif rescale_w and rescale_h and keep_aspect_ratio:
            ratio = min(pad_h / src_h, pad_w / src_w)
            new_w, new_h, filt = int(src_w * ratio), int(src_h * ratio), BICUBIC
        elif rescale_w and not rescale_h:
            if src_w != pad_w:
                new_w, new_h, filt = pad_w, int(src_h * (pad_w / src_w)), BICUBIC
        elif rescale_h and not rescale_w:
            if src_h != pad_h:
                new_w, new_h, filt = int(src_w * (pad_h / src_h)), pad_h, BICUBIC
    if new_w <= 0 or new_h <= 0:
        raise ValueError("height and width must be > 0")     # (Pillow's, from Image.resize)
    if (new_w, new_h) == (src_w, src_h):
        filt = None                                           # Image.resize returns a copy
    # _crop: the left / upper shift is half the difference, an odd difference loses one more pixel at the far side
    crop_x, crop_y = max(new_w - pad_w, 0) // 2, max(new_h - pad_h, 0) // 2
    return Geometry(src_w, src_h, new_w, new_h, filt, crop_x, crop_y, min(new_w, pad_w), min(new_h, pad_h))


def tables_of(geometry: Geometry) -> Tuple[Table, Table]:
    """The (horizontal, vertical) tables of the outputs that survive the crop."""
    g = geometry
    if g.filt is None:
        across, down = identity_table(g.new_w), identity_table(g.new_h)
    else:
        across = resample_table(g.src_w, g.new_w, g.filt) if g.new_w != g.src_w else identity_table(g.new_w)
        down = resample_table(g.src_h, g.new_h, g.filt) if g.new_h != g.src_h else identity_table(g.new_h)
    return across.keep(g.crop_x, g.copy_w), down.keep(g.crop_y, g.copy_h)


class ChunkPlan:
    """The arrays of include/nmhip_imgread.h for a chunk of decoded images (``uint8`` ``[h, w]`` or ``[h, w, 3]``)."""

    def __init__(self, images: List[np.ndarray], geometries: List[Geometry], mode: str, pad_w: int, pad_h: int) -> None:
        assert len(images) == len(geometries) >= 1
        self.mode, self.target, self.pad_w, self.pad_h = mode, DEVICE_MODES[mode], pad_w, pad_h
        self.channels = MODE_CHANNELS[mode]
        n = len(images)
        self.offs = np.zeros((6, n + 1), np.int64)
        self.geom = np.zeros((n, 16), np.int32)
        flat, across_all, down_all = [], [], []
        for i, (image, g) in enumerate(zip(images, geometries)):
            bands = 1 if image.ndim == 2 else image.shape[2]
            if image.dtype != np.uint8 or bands not in (1, 3) or image.shape[:2] != (g.src_h, g.src_w):
                raise ValueError("a decoded image must be uint8 [h, w] or [h, w, 3], not {} {}".format(image.dtype,
                                                                                                     image.shape))
            across, down = tables_of(g)
            row0 = int(down.first.min()) if g.copy_h else 0
            rows = int((down.first + down.count).max()) - row0 if g.copy_h else 0
            self.geom[i, :13] = (g.src_w, g.src_h, bands, g.new_w, g.new_h, g.crop_x, g.crop_y, g.copy_w, g.copy_h, row0,
                                 rows, across.k.shape[1], down.k.shape[1])
            flat.append(np.ascontiguousarray(image).reshape(-1))
            across_all.append(across)
            down_all.append(down)
            self.offs[0, i + 1] = self.offs[0, i] + flat[-1].size
            self.offs[1, i + 1] = self.offs[1, i] + rows * g.copy_w * self.channels
            self.offs[2, i + 1] = self.offs[2, i] + g.copy_w
            self.offs[3, i + 1] = self.offs[3, i] + across.k.size
        self.offs[4, 0], self.offs[5, 0] = self.offs[2, n], self.offs[3, n]      # the vertical tables follow
        for i, down in enumerate(down_all):
            self.offs[4, i + 1] = self.offs[4, i] + down.first.size
            self.offs[5, i + 1] = self.offs[5, i] + down.k.size
        both = across_all + down_all
        self.src = np.concatenate(flat)
        self.bounds = np.ascontiguousarray(np.stack([np.concatenate([t.first for t in both]),
                                                     np.concatenate([t.count for t in both])], axis=1).astype(np.int32))
        k = np.concatenate([t.k.reshape(-1) for t in both])
        self.coef = np.ascontiguousarray(k if mode == "F" else fixed_point(k))
        self.scratch_elems = int(self.offs[1, n])
        self.max_rows = int(self.geom[:, 10].max())

    def run(self, sub: Optional[np.ndarray] = None, divide: float = 1.0, out=None) -> np.ndarray:
        """The device pipeline: upload, two launches, copy back -> float32 ``[N, pad_h, pad_w, channels]``."""
        import torch
        from .. import ops
        if not torch.cuda.is_available():
            raise RuntimeError("readers.image_reader resizes, crops and pads on the GPU; none is visible (there is no "
                               "host fallback)")
        ops.imgread_check(self.offs, self.geom, self.target, self.pad_w, self.pad_h)
        device = torch.device("cuda", torch.cuda.current_device())
        d = {name: torch.from_numpy(getattr(self, name)).to(device) for name in ("src", "offs", "geom", "bounds", "coef")}
        scratch = torch.empty(max(self.scratch_elems, 1), dtype=torch.float32 if self.mode == "F" else torch.uint8,
                              device=device)
        if out is None:
            out = torch.empty((len(self.geom), self.pad_h, self.pad_w, self.channels), dtype=torch.float32, device=device)
        d_sub = None if sub is None else torch.from_numpy(np.ascontiguousarray(sub, np.float64).reshape(-1)).to(device)
        ops.imgread_rows(d["src"], d["offs"], d["geom"], d["bounds"], d["coef"], self.target, self.pad_w, self.max_rows,
                         scratch)
        ops.imgread_cols(scratch, d["offs"], d["geom"], d["bounds"], d["coef"], self.target, out, d_sub, divide)
        return out.cpu().numpy()


# ---- decoding -------------------------------------------------------------------------------------------------------------
def parse_pnm(data: bytes) -> Optional[np.ndarray]:
    """A binary PGM (``P5``) or PPM (``P6``) file with maxval 255 -> uint8 ``[h, w]`` / ``[h, w, 3]``; None for
    anything else (which then goes to Pillow)."""
    if data[:2] not in (b"P5", b"P6"):
        return None
    bands = 1 if data[:2] == b"P5" else 3
    fields, pos = [], 2
    while len(fields) < 3:
        while pos < len(data) and data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":                           # a comment runs to the end of its line
            while pos < len(data) and data[pos:pos + 1] not in (b"\n", b"\r"):
                pos += 1
            continue
        start = pos
        while pos < len(data) and data[pos:pos + 1].isdigit():
            pos += 1
        if pos == start:
            return None
        fields.append(int(data[start:pos]))
    width, height, maxval = fields
    pos += 1                                                    # the single whitespace byte before the raster
    if maxval != 255 or width < 1 or height < 1 or len(data) - pos < width * height * bands:
        return None
    raster = np.frombuffer(data, np.uint8, width * height * bands, pos)
    return raster.reshape((height, width) if bands == 1 else (height, width, 3)).copy()


def _pillow():
    try:
        from PIL import Image, ImageFile
    except ImportError as exc:
        raise ImportError("readers.image_reader decodes image files with Pillow (PIL), which is not installed; only "
                          "binary PGM / PPM files can be read without it") from exc
    ImageFile.LOAD_TRUNCATED_IMAGES = True
    return Image


def decode(path: str) -> np.ndarray:
    """The file's pixels as 8-bit ``L`` or ``RGB``: what ``Image.open(path)`` holds, one-band modes converted to ``L``
    and every other mode to ``RGB`` on the host.  Raises IOError for a file Pillow cannot read."""
    with open(path, "rb") as handle:
        data = handle.read()
    pixels = parse_pnm(data)
    if pixels is not None:
        return pixels
    image = _pillow().open(path)
    if image.mode not in ("L", "RGB"):
        image = image.convert("L" if len(image.getbands()) == 1 else "RGB")
    return np.array(image)


def _paths(list_files: List[str], prefix: str, base: str, message: str) -> Iterator[Tuple[int, str, str]]:
    """(line number, the path as the reference would print it, the path to open) of every listed file.  ``base`` is
    ``prefix`` made absolute when the reader was built: a lazy dataset opens its files when it is iterated, wherever the
    process stands by then."""
    for list_file in list_files:
        with open(list_file) as f_list:
            for i, image_file in enumerate(f_list):
                shown, path = os.path.join(prefix, image_file.rstrip()), os.path.join(base, image_file.rstrip())
                if not os.path.exists(path):
                    raise Exception(message.format(shown, i + 1))
                yield i, shown, path


def _chunked(items: Iterator, process: Callable[[List], np.ndarray]) -> Iterator[np.ndarray]:
    """``process`` over chunks of ``items`` (image, geometry), rows yielded one by one.  An error while the next item
    is read is raised after the images before it have been yielded, as a reader that works image by image would."""
    pending, pixels, failure = [], 0, None
    while failure is None:
        try:
            item = next(items)
        except StopIteration:
            break
        except Exception as exc:           # pylint: disable=broad-except
            failure = exc
            break
        pending.append(item)
        pixels += item[0].shape[0] * item[0].shape[1]
        if len(pending) >= CHUNK_IMAGES or pixels >= CHUNK_PIXELS:
            yield from process(pending)
            pending, pixels = [], 0
    if pending:
        yield from process(pending)
    if failure is not None:
        raise failure


def image_reader(pad_w: int,
                 pad_h: int,
                 channels: int = 3,
                 prefix: str = "",
                 rescale_w: bool = False,
                 rescale_h: bool = False,
                 keep_aspect_ratio: bool = False,
                 mode: str = "RGB") -> Callable:
    """A reader for a dataset series of images.  Every image is converted to ``mode`` ("L", "RGB" or "F"), brought to
    ``pad_w`` x ``pad_h`` and yielded as a float32 array ``[pad_h, pad_w, channels]``; ``channels`` must be what the
    mode has (3 for "RGB", else 1).  A side whose ``rescale_*`` flag is set is resized to its target, the other one is
    centre-cropped where it is too long and zero-padded at the right / bottom where it is too short.  Both sides
    without ``keep_aspect_ratio`` stretch the image (BILINEAR); with it the image is scaled by one ratio (BICUBIC) --
    the smaller of the two when both sides are rescaled -- and then cropped / padded.  One side alone requires
    ``keep_aspect_ratio``; ``keep_aspect_ratio`` alone is refused.  ``prefix`` is joined in front of every listed path.
    """
    check_argument_types()
    if not rescale_w and not rescale_h and keep_aspect_ratio:
        raise ValueError("It does not make sense to keep the aspect ratio while not rescaling the image.")
    if rescale_w != rescale_h and not keep_aspect_ratio:
        raise ValueError("While rescaling only one side, aspect ratio must be kept, was set to false.")
    if mode not in DEVICE_MODES:
        raise NotImplementedError("image_reader: mode '{}' is not computed on the device (only {})".format(
            mode, ", ".join("'{}'".format(m) for m in DEVICE_MODES)))
    if pad_w < 1 or pad_h < 1:
        raise ValueError("image_reader: pad_w {} and pad_h {} must be at least 1".format(pad_w, pad_h))
    base = os.path.abspath(prefix)

    def decoded(list_files: List[str]) -> Iterator[Tuple[np.ndarray, Geometry]]:
        for i, shown, path in _paths(list_files, prefix, base, "Image file '{}' no.{}  does not exist."):
            try:
                pixels = decode(path)
            except IOError:
                warn("Skipping image from file '{}' no. '{}'.".format(shown, i + 1))
                pixels = np.zeros((pad_h, pad_w), np.uint8)            # Image.new(mode, (pad_w, pad_h))
            if pixels.ndim not in (2, 3):
                raise ValueError("Image should have either 2 (black and white) or three dimensions (color channels), "
                                 "has {} dimension.".format(pixels.ndim))
            img_channels = MODE_CHANNELS[mode]
            if channels != img_channels:
                raise ValueError("Image does not have the pre-declared number of channels {}, but {}.".format(
                    channels, img_channels))
            yield pixels, plan_image(pixels.shape[1], pixels.shape[0], pad_w, pad_h, rescale_w, rescale_h,
                                     keep_aspect_ratio)

    def process(chunk: List[Tuple[np.ndarray, Geometry]]) -> np.ndarray:
        return ChunkPlan([c[0] for c in chunk], [c[1] for c in chunk], mode, pad_w, pad_h).run()

    def load(list_files: List[str]) -> Iterable[np.ndarray]:
        return _chunked(decoded(list_files), process)

    return load


def _imagenet_geometry(pixels: np.ndarray, target_width: int, target_height: int) -> Geometry:
    """The reference resizes and DISCARDS the result (readers/image_reader.py:154-165 do not assign it): the array is
    the image centre-cropped and zero-padded."""
    return plan_image(pixels.shape[1], pixels.shape[0], target_width, target_height, False, False, False)


def _imagenet_epilogue(vgg_normalization: bool, zero_one_normalization: bool):
    sub = np.array(VGG_RGB_MEANS, np.float64).reshape(3) if vgg_normalization else None
    return sub, 255.0 if zero_one_normalization else 1.0


def _check_imagenet_shape(target_width: int, target_height: int) -> None:
    # the reference asserts the [h, w, 3] array against (w, h, 3)
    assert (target_height, target_width, 3) == (target_width, target_height, 3)


def imagenet_reader(prefix: str,
                    target_width: int = 227,
                    target_height: int = 227,
                    vgg_normalization: bool = False,
                    zero_one_normalization: bool = False) -> Callable:
    """A reader for ImageNet-style networks: every image as RGB, centre-cropped and zero-padded to ``target_width`` x
    ``target_height`` (which must be equal, see ``_check_imagenet_shape``), as a float32 array; ``vgg_normalization``
    subtracts ``VGG_RGB_MEANS`` per channel, ``zero_one_normalization`` then divides by 255.  ``prefix`` is joined in
    front of every listed path."""
    check_argument_types()
    sub, divide = _imagenet_epilogue(vgg_normalization, zero_one_normalization)
    base = os.path.abspath(prefix)

    def decoded(list_files: List[str]) -> Iterator[Tuple[np.ndarray, Geometry]]:
        for _, _, path in _paths(list_files, prefix, base, "Image file '{}' no. {} does not exist."):
            pixels = decode(path)
            _check_imagenet_shape(target_width, target_height)
            yield pixels, _imagenet_geometry(pixels, target_width, target_height)

    def process(chunk: List[Tuple[np.ndarray, Geometry]]) -> np.ndarray:
        plan = ChunkPlan([c[0] for c in chunk], [c[1] for c in chunk], "RGB", target_width, target_height)
        return plan.run(sub, divide)

    def load(list_files: List[str]) -> Iterable[np.ndarray]:
        return _chunked(decoded(list_files), process)

    return load


def single_image_for_imagenet(path: str, target_height: int, target_width: int, vgg_normalization: bool,
                              zero_one_normalization: bool) -> np.ndarray:
    """One file through ``imagenet_reader``'s pipeline."""
    pixels = decode(path)
    _check_imagenet_shape(target_width, target_height)
    sub, divide = _imagenet_epilogue(vgg_normalization, zero_one_normalization)
    plan = ChunkPlan([pixels], [_imagenet_geometry(pixels, target_width, target_height)], "RGB", target_width,
                     target_height)
    return plan.run(sub, divide)[0]
