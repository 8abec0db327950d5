"""Pre-trained ImageNet networks (mirror of neuralmonkey/encoders/imagenet_encoder.py).

``ImageNet`` runs TF-slim's VGG-16 or VGG-19 (nets/vgg.py with ``is_training=False`` and keep probability 1) over
[B, 224, 224, 3] images whose VGG means the reader has subtracted, and hands one of its convolutional maps to an attention
(``spatial_states``) and one vector per image to a decoder (``output``).  TF-slim is not imported: the network is restated
here from its published definition --

  conv1 .. conv5   2, 2, 3, 3, 3 (vgg_16) or 2, 2, 4, 4, 4 (vgg_19) convolutions 3 x 3, stride 1, SAME, + bias + ReLU, of
                   64, 128, 256, 512, 512 channels; every block ends with poolN: 2 x 2 max, stride 2, VALID
  fc6              7 x 7 VALID convolution to 4096 + ReLU; fc7: 1 x 1 to 4096 + ReLU; fc8: 1 x 1 to 1000, no activation

with slim's endpoint keys (``<net>/convN/convN_M``, ``<net>/poolN``, ``<net>/fc6``, ``<net>/fc7`` and ``<net>/fc8``,
which slim squeezes to [B, 1000]) and variable names (``<endpoint>/weights`` [k, k, Cin, Cout], ``<endpoint>/biases``).

The network is frozen: the reference wraps what it hands on in ``tf.stop_gradient`` (:212, :234), so ``backward`` does
nothing, and its variables are declared non-trainable under slim's own names -- ``vgg_16/...``, whatever the part is
called (the reference's docstring: "will be in its scope, independently on `name`"; its saver collects
``scope=self.network_type``, :242-243) -- so that a slim checkpoint loads, no optimizer holds slots for them and no
regulariser moves them.  Only the layers up to the deepest endpoint the part uses are declared and computed.

MI355X mapping: every 3 x 3 convolution is one launch of csrc/nm_vgg.hip (``ops.conv2d_act_fwd``: implicit GEMM over the
flattened positions on the fp32 matrix cores with bias and ReLU on the accumulators); ``conv_route`` sends a layer shape
to the image stack's ``conv2d_fwd`` + a ReLU pass instead where tools/bench_vgg.py measured that faster.  Pooling is
``window2d_fwd``; fc6 .. fc8 are plain products on ``ops.gemm`` with its bias / ReLU epilogue (the NHWC flattening of the
7 x 7 x 512 map is the filter's (ky, kx, ci) order)."""
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from .. import ops
from ..checking import check_argument_types
from ..model.model_part import FeedDict, InitializerSpecs, ModelPart
from ..model.stateful import SpatialStatefulWithOutput
from ..runtime import Placeholder, tensor
from ..variables import zeros_initializer
from .sentence_cnn_encoder import conv_filter_initializer

IMAGE_SIZE = (224, 224)

# convolutions per block
VGG_BLOCKS = {"vgg_16": (2, 2, 3, 3, 3), "vgg_19": (2, 2, 4, 4, 4)}
# widths as data, one table per network: the five blocks' channels, fc6 and fc7, the classes of fc8.  The layer lists are
# derived from these on every use.
NETWORK_WIDTHS = {
    "vgg_16": {"conv": (64, 128, 256, 512, 512), "fc": (4096, 4096), "classes": 1000},
    "vgg_19": {"conv": (64, 128, 256, 512, 512), "fc": (4096, 4096), "classes": 1000},
}

_NOT_BUILT = ("Network '{}' is not built on this engine: it would need strided convolutions and inference-mode batch "
              "normalisation over residual units (vgg_16 and vgg_19 are built)")

# the reference's keys, in its order; None: refused at construction
SUPPORTED_NETWORKS = {
    "alexnet_v2": None,
    "vgg_16": "vgg_16",
    "vgg_19": "vgg_19",
    "resnet_v2_50": None,
    "resnet_v2_101": None,
    "resnet_v2_152": None,
}


class Layer(NamedTuple):
    endpoint: str
    kind: str                          # "conv" (3 x 3 SAME), "pool" (2 x 2 / 2 VALID) or "fc" (k x k VALID on a k x k map)
    k: int
    cin: int
    cout: int
    relu: bool
    in_hw: Tuple[int, int]
    out_hw: Tuple[int, int]

    @property
    def variables(self) -> List[Tuple[str, Tuple[int, ...]]]:
        if self.kind == "pool":
            return []
        return [(self.endpoint + "/weights", (self.k, self.k, self.cin, self.cout)),
                (self.endpoint + "/biases", (self.cout,))]

    @property
    def out_shape(self) -> Tuple[int, ...]:
        """The endpoint's shape behind the batch axis."""
        if self.endpoint.endswith("/fc8"):
            return (self.cout,)                                    # slim squeezes the logits
        return self.out_hw + (self.cout,)


def layer_table(network_type: str, image_size: Tuple[int, int] = IMAGE_SIZE) -> List[Layer]:
    """The network's layers in order, with their static shapes, from ``NETWORK_WIDTHS``."""
    widths = NETWORK_WIDTHS[network_type]
    (h, w), cin = image_size, 3
    layers = []
    for n, (count, cout) in enumerate(zip(VGG_BLOCKS[network_type], widths["conv"]), start=1):
        for m in range(1, count + 1):
            layers.append(Layer("{}/conv{}/conv{}_{}".format(network_type, n, n, m), "conv", 3, cin, cout, True,
                                (h, w), (h, w)))
            cin = cout
        layers.append(Layer("{}/pool{}".format(network_type, n), "pool", 2, cin, cin, False, (h, w), (h // 2, w // 2)))
        h, w = h // 2, w // 2
    assert h == w == 7, "fc6 is a 7 x 7 convolution over pool5"
    fc6, fc7 = widths["fc"]
    layers.append(Layer(network_type + "/fc6", "fc", 7, cin, fc6, True, (h, w), (1, 1)))
    layers.append(Layer(network_type + "/fc7", "fc", 1, fc6, fc7, True, (1, 1), (1, 1)))
    layers.append(Layer(network_type + "/fc8", "fc", 1, fc7, widths["classes"], False, (1, 1), (1, 1)))
    return layers


def parameter_count(network_type: str, upto: Optional[str] = None) -> int:
    """Parameters of the layers up to the endpoint ``upto`` (the whole network by default), from the table alone."""
    total = 0
    for layer in layer_table(network_type):
        total += sum(int(np.prod(shape)) for _, shape in layer.variables)
        if layer.endpoint == upto:
            break
    return total


def conv_route(bsz: int, layer: Layer) -> str:
    """Which kernel runs a 3 x 3 layer of this shape: "act" (nm_conv2d_act_fwd) or "conv2d+relu" (nm_conv2d_fwd and a
    ReLU pass).  tools/bench_vgg.py measured both on every VGG-16 layer shape at B = 5 and B = 32 (DESIGN.md section
    4.20): the fused kernel was faster on all of them, so nothing is routed to the older pair."""
    del bsz, layer
    return "act"


def run_layers(plan: List[Layer], images: torch.Tensor, variable, buffer, route=conv_route) -> Dict[str, torch.Tensor]:
    """The layers of ``plan`` over ``images`` [B, H, W, 3]: endpoint -> tensor ([B, H, W, C]; ``<net>/fc8``
    [B, classes]).  ``variable(full name)`` hands out a variable, ``buffer(endpoint, shape)`` the endpoint's output
    buffer, ``route(batch, layer)`` names the kernel of a 3 x 3 layer."""
    x = images
    bsz = int(x.shape[0])
    ends = {}
    for layer in plan:
        out = buffer(layer.endpoint, (bsz,) + layer.out_hw + (layer.cout,))
        if layer.kind == "pool":
            ops.window2d_fwd("max", x, out, (2, 2), (2, 2), "valid")
        else:
            filt, bias = variable(layer.variables[0][0]), variable(layer.variables[1][0])
            if layer.kind == "fc":
                depth = layer.k * layer.k * layer.cin
                ops.gemm(x.view(bsz, depth), filt.view(depth, layer.cout), out=out.view(bsz, layer.cout), bias=bias,
                         act="relu" if layer.relu else None)
            elif route(bsz, layer) == "act":
                ops.conv2d_act_fwd(x, filt, bias, out, "same", relu=layer.relu)
            else:
                ops.conv2d_fwd(x, filt, bias, out, "same")
                if layer.relu:
                    flat = out.view(-1, layer.cout)
                    ops.ew("relu", flat, None, flat)
        x = out
        ends[layer.endpoint] = out.view((bsz,) + layer.out_shape)
    return ends


# pylint: disable=too-many-instance-attributes
class ImageNet(ModelPart, SpatialStatefulWithOutput):
    """Pre-trained ImageNet network (frozen)."""
    has_time_loop = False

    # pylint: disable=too-many-arguments
    def __init__(self,
                 name: str,
                 data_id: str,
                 network_type: str,
                 slim_models_path: str,
                 load_checkpoint: str = None,
                 spatial_layer: str = None,
                 encoded_layer: str = None,
                 initializers: InitializerSpecs = None) -> None:
        """``slim_models_path`` is accepted and ignored: nothing under it is imported or run."""
        check_argument_types()
        ModelPart.__init__(self, name, load_checkpoint=load_checkpoint, initializers=initializers, save_checkpoint=None)

        self.data_id = data_id
        self.network_type = network_type
        self.spatial_layer = spatial_layer
        self.encoded_layer = encoded_layer

        if self.network_type not in SUPPORTED_NETWORKS:
            raise ValueError(
                "Network '{}' is not among the supported ones ({})".format(
                    self.network_type, ", ".join(SUPPORTED_NETWORKS.keys())))
        if SUPPORTED_NETWORKS[self.network_type] is None:
            raise NotImplementedError(_NOT_BUILT.format(self.network_type))

        # the variables live in slim's scope, not in the part's
        self._scope = self.network_type
        self._initializer_overrides = {"{}/{}".format(self._scope, var_name): init
                                       for var_name, init in (initializers or [])}
        self.height, self.width = IMAGE_SIZE
        self.image_input = Placeholder("{}/input_image".format(name))
        self._plan = self._lay_out()
    # pylint: enable=too-many-arguments

    def _lay_out(self) -> List[Layer]:
        """The layers up to the deepest endpoint in use, after the reference's checks of the two endpoint names."""
        layers = layer_table(self.network_type, (self.height, self.width))
        by_name = {layer.endpoint: layer for layer in layers}
        if self.spatial_layer is not None and self.spatial_layer not in by_name:
            raise ValueError(
                "Network '{}' does not contain endpoint '{}'".format(
                    self.network_type, self.spatial_layer))
        if self.spatial_layer is not None:
            shape = by_name[self.spatial_layer].out_shape
            if len(shape) != 3:
                raise ValueError(
                    "Endpoint '{}' for network '{}' cannot be a convolutional "
                    " map, its dimensionality is: {}.".format(
                        self.spatial_layer, self.network_type,
                        ", ".join(["None"] + [str(d) for d in shape])))
        if self.encoded_layer is not None and self.encoded_layer not in by_name:
            raise ValueError(
                "Network '{}' does not contain endpoint '{}'.".format(
                    self.network_type, self.encoded_layer))
        # ... and where the reference would fail inside TensorFlow
        if self.spatial_layer is None and self.encoded_layer is None:
            raise ValueError("ImageNet '{}': one of spatial_layer and encoded_layer must be given (the output would be "
                             "the mean of a map that is not there)".format(self.name))
        if self.encoded_layer is not None:
            shape = by_name[self.encoded_layer].out_shape
            if len(shape) != 3:
                raise ValueError("ImageNet '{}': encoded_layer '{}' is {}-dimensional, its map axes cannot be squeezed "
                                 "away ('{}/fc8' is squeezed by the network itself)"
                                 .format(self.name, self.encoded_layer, len(shape) + 1, self.network_type))
            if shape[:2] != (1, 1):
                raise ValueError("ImageNet '{}': encoded_layer '{}' is a {} x {} map, only a 1 x 1 map can be squeezed "
                                 "to a vector".format(self.name, self.encoded_layer, shape[0], shape[1]))
        used = [n for n in (self.spatial_layer, self.encoded_layer) if n is not None]
        last = max(i for i, layer in enumerate(layers) if layer.endpoint in used)
        return layers[:last + 1]

    def _layer(self, endpoint: str) -> Layer:
        return next(layer for layer in self._plan if layer.endpoint == endpoint)

    @property
    def input_types(self) -> Dict[str, type]:
        return {self.data_id: np.float32}

    @property
    def input_shapes(self) -> Dict[str, List]:
        return {self.data_id: [None, self.height, self.width, 3]}

    @property
    def dimension(self) -> int:
        if self.spatial_layer is None:
            raise ValueError("ImageNet '{}' has no spatial_layer".format(self.name))
        return self._layer(self.spatial_layer).cout

    @property
    def output_size(self) -> int:
        return self._layer(self.encoded_layer).cout if self.encoded_layer is not None else self.dimension

    def graph_safe_training(self, train_mode: bool) -> bool:
        """The images are staged from the host on every step and nothing here is trained: the step's graph starts
        behind this part."""
        return False

    # -- variables ---------------------------------------------------------------------------------------------
    def declare_variables(self, store) -> None:
        prefix = self._scope + "/"
        for layer in self._plan:
            for full, shape in layer.variables:
                init = conv_filter_initializer() if full.endswith("/weights") else zeros_initializer()
                self.declare(store, full[len(prefix):], shape, init, trainable=False)

    # -- inputs -------------------------------------------------------------------------------------------------
    def feed_dict(self, dataset, train: bool = False) -> FeedDict:
        fd = ModelPart.feed_dict(self, dataset, train)
        images = np.array(list(dataset.get_series(self.data_id)))
        assert images.shape[1:] == (self.height, self.width, 3)
        fd[self.image_input] = images.astype(np.float32, copy=False)
        return fd

    @tensor
    def input_image(self, ctx) -> torch.Tensor:
        """The fed images in a persistent device buffer."""
        images = ctx.fed(self.image_input)
        return ctx.session.staged((id(self), "images"), ctx.session.to_device(images, torch.float32, "input_image"))

    def stage_inputs(self, ctx) -> None:
        self.input_image(ctx)

    # -- forward ------------------------------------------------------------------------------------------------
    @tensor
    def end_points(self, ctx) -> Dict[str, torch.Tensor]:
        """endpoint -> tensor for every layer the part computes ([B, H, W, C]; ``<net>/fc8`` [B, classes])."""
        x = self.input_image(ctx)
        bsz = int(x.shape[0])
        return run_layers(self._plan, x, lambda full: ctx.store[full],
                          lambda endpoint, shape: ctx.buffer((id(self), endpoint, bsz), shape))

    @tensor
    def spatial_states(self, ctx) -> Optional[torch.Tensor]:
        if self.spatial_layer is None:
            return None
        return self.end_points(ctx)[self.spatial_layer]

    @tensor
    def spatial_mask(self, ctx) -> Optional[torch.Tensor]:
        if self.spatial_layer is None:
            return None
        shape = tuple(self.spatial_states(ctx).shape[:3])
        mask = ctx.buffer((id(self), "mask", shape), shape)
        ops.fill(mask, 1.0)
        return mask

    @tensor
    def output(self, ctx) -> torch.Tensor:
        if self.encoded_layer is None:
            states = self.spatial_states(ctx)                      # tf.reduce_mean(states, [1, 2])
            bsz, h, w, c = states.shape
            out = ctx.buffer((id(self), "output", bsz), (bsz, 1, 1, c))
            ops.window2d_fwd("avg", states, out, (h, w), (1, 1), "valid")
            return out.view(bsz, c)
        encoded = self.end_points(ctx)[self.encoded_layer]         # tf.squeeze(., [1, 2])
        return encoded.view(encoded.shape[0], encoded.shape[3])

    def backward(self, ctx, d_states: Optional[torch.Tensor], d_final: Optional[torch.Tensor] = None) -> None:
        """tf.stop_gradient: nothing behind the states and the output receives a gradient."""
