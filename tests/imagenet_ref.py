"""TF-slim's VGG-16 / VGG-19 (nets/vgg.py, ``is_training=False``, keep probability 1) restated on
``torch.nn.functional.conv2d`` and ``max_pool2d`` on the CPU, in float64 by default: the reference of
tests/test_imagenet_kernels_gpu.py and tests/test_imagenet_gpu.py.  Neither the engine nor its authors wrote the
convolution that runs here.  Maps are NHWC arrays, filters TensorFlow's [k, k, Cin, Cout], variables under slim's names
(``<net>/convN/convN_M/weights`` ...).  The layer list is written out here on its own, not derived from the engine's
width table; only the widths are passed in, because the tests run narrow networks."""
import numpy as np
import torch
import torch.nn.functional as F

BLOCKS = {"vgg_16": (2, 2, 3, 3, 3), "vgg_19": (2, 2, 4, 4, 4)}
WIDTHS = {"conv": (64, 128, 256, 512, 512), "fc": (4096, 4096), "classes": 1000}


def same_pads(k):
    """(before, after) of TensorFlow's SAME padding at stride 1."""
    return (k - 1) // 2, k - 1 - (k - 1) // 2


def conv2d(x, filt, bias, padding, relu, dtype=torch.float64):
    """x [B, H, W, Cin] (array), filt [k, k, Cin, Cout], bias [Cout] or None -> [B, OH, OW, Cout] array of ``dtype``."""
    xt = torch.as_tensor(np.asarray(x)).to(dtype).permute(0, 3, 1, 2)
    wt = torch.as_tensor(np.asarray(filt)).to(dtype).permute(3, 2, 0, 1)
    k = wt.shape[2]
    if padding == "same":
        before, after = same_pads(k)
        xt = F.pad(xt, (before, after, before, after))
    out = F.conv2d(xt, wt, None if bias is None else torch.as_tensor(np.asarray(bias)).to(dtype))
    if relu:
        out = torch.relu(out)
    return out.permute(0, 2, 3, 1).contiguous().numpy()


def max_pool(x, dtype=torch.float64):
    xt = torch.as_tensor(np.asarray(x)).to(dtype).permute(0, 3, 1, 2)
    return F.max_pool2d(xt, 2, 2).permute(0, 2, 3, 1).contiguous().numpy()


def layers(net, widths=None):
    """[(endpoint, kind, k, padding, Cin, Cout, relu)] in order; kind "conv" or "pool" (k, padding, relu unused)."""
    widths = widths or WIDTHS
    out, cin = [], 3
    for n, (count, cout) in enumerate(zip(BLOCKS[net], widths["conv"]), start=1):
        for m in range(1, count + 1):
            out.append(("{}/conv{}/conv{}_{}".format(net, n, n, m), "conv", 3, "same", cin, cout, True))
            cin = cout
        out.append(("{}/pool{}".format(net, n), "pool", 2, "valid", cin, cin, False))
    out.append((net + "/fc6", "conv", 7, "valid", cin, widths["fc"][0], True))
    out.append((net + "/fc7", "conv", 1, "valid", widths["fc"][0], widths["fc"][1], True))
    out.append((net + "/fc8", "conv", 1, "valid", widths["fc"][1], widths["classes"], False))
    return out


def random_variables(net, widths, seed, upto=None):
    """Glorot-scaled random filters and random biases of both signs, float32, for the layers up to ``upto``."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, kind, k, _, cin, cout, _ in layers(net, widths):
        if kind == "conv":
            lim = np.sqrt(6.0 / (k * k * (cin + cout)))
            out[name + "/weights"] = rng.uniform(-lim, lim, (k, k, cin, cout)).astype(np.float32)
            out[name + "/biases"] = rng.uniform(-0.1, 0.1, (cout,)).astype(np.float32)
        if name == upto:
            break
    return out


def forward(net, variables, images, widths=None, upto=None, dtype=torch.float64):
    """endpoint -> array for every layer up to ``upto`` (all of them by default); fc8 squeezed to [B, classes]."""
    x, ends = np.asarray(images), {}
    for name, kind, _, padding, _, _, relu in layers(net, widths):
        if kind == "pool":
            x = max_pool(x, dtype)
        else:
            x = conv2d(x, variables[name + "/weights"], variables[name + "/biases"], padding, relu, dtype)
        ends[name] = x
        if name == upto:
            break
    if net + "/fc8" in ends:
        ends[net + "/fc8"] = ends[net + "/fc8"][:, 0, 0, :]
    return ends
