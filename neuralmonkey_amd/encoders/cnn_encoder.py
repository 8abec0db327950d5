"""CNN for image processing (mirror of neuralmonkey/encoders/cnn_encoder.py).

``CNNEncoder``: images [B, H, W, pixel_dim] / 255 (:204-205) through a list of layers -- ``("C", k, stride, pad, n)``
tf.layers.conv2d + batch norm + ReLU (:231-236; the convolution IGNORES the stride, only the mask's max-pool uses it,
:238), ``("M" | "A", size, stride, pad)`` max / average pooling (:318-319; the padding is validated and NOT passed on, so
maps and mask pool VALID), ``("R", k, n)`` a pre-activation residual block (:260-284; the mask passes through).  The
mask is sign(sum over the channels of the image) (:103), max-pooled along with the maps.  ``output`` is the unmasked
mean of the last map (:187) or, with ``fully_connected``, the flattened map through ``multilayer_projection`` (:190-197).
``CNNTemporalView`` cuts the last map into its columns: ``temporal_states`` [B, W', H'*C'] (:340-344), ``temporal_mask``
= (sum over H' of the mask) > 0 (:348-350).

MI355X mapping: every layer is one or two launches of csrc/nm_image.hip through the taped functions of ``image_ops``
(an implicit-GEMM convolution on the fp32 matrix cores or a scalar kernel, a two-pass batch norm with the ReLU in its
second pass, gather-style pooling); the masks -- the image's is derived on the host from the fed pixels -- go through
the same pooling kernel with one channel.  The moving statistics of the batch norms are non-trainable variables that the
forward pass of a trainer's step updates in place (the reference's trainers fetch UPDATE_OPS: generic_trainer.py:250);
a runner's pass never touches them.  Everything is recorded on an autodiff tape; ``backward`` replays it.
"""
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from .. import autodiff as F
from .. import image_ops as I
from .. import ops
from ..checking import check_argument_types, matches
from ..model.model_part import FeedDict, InitializerSpecs, ModelPart
from ..model.stateful import SpatialStatefulWithOutput, TemporalStatefulWithOutput
from ..nn import mlp
from ..runtime import Placeholder, tensor
from ..variables import ones_initializer, zeros_initializer
from .sentence_cnn_encoder import conv_filter_initializer

# pylint: disable=invalid-name
ConvSpec = Tuple[str, int, int, str, int]
ResNetSpec = Tuple[str, int, int]
MaxPoolSpec = Tuple[str, int, int, str]
# pylint: enable=invalid-name

MLP_SCOPE = "mlp"            # nn/projection.py:44, multilayer_projection's default scope


def _check_padding(pad: str, layer_num: int) -> None:
    if pad not in ["same", "valid"]:
        raise ValueError(("Padding must be 'same' or 'valid', "
                          "was '{}' in layer {}.").format(pad, layer_num + 1))


# pylint: disable=too-many-instance-attributes
class CNNEncoder(ModelPart, SpatialStatefulWithOutput):
    """An image encoder."""
    has_time_loop = False

    # pylint: disable=too-many-arguments, too-many-locals
    def __init__(self,
                 name: str,
                 data_id: str,
                 convolutions: List[Union[ConvSpec, ResNetSpec, MaxPoolSpec]],
                 image_height: int, image_width: int, pixel_dim: int,
                 fully_connected: List[int] = None,
                 batch_normalize: bool = False,
                 dropout_keep_prob: float = 0.5,
                 reuse: ModelPart = None,
                 save_checkpoint: str = None,
                 load_checkpoint: str = None,
                 initializers: InitializerSpecs = None) -> None:
        check_argument_types()
        ModelPart.__init__(self, name, reuse, save_checkpoint, load_checkpoint, initializers)

        self.data_id = data_id
        self.dropout_keep_prob = dropout_keep_prob

        self.image_height = image_height
        self.image_width = image_width
        self.pixel_dim = pixel_dim
        self.convolutions = convolutions
        self.fully_connected = fully_connected
        self.batch_normalize = batch_normalize

        self.image_input = Placeholder("{}/image_input".format(name))
        # the reference meets a bad specification when it builds its graph; here the layers are laid out right away
        self._plan = self._lay_out()
    # pylint: enable=too-many-arguments, too-many-locals

    # -- the layers, with their static shapes --------------------------------------------------------------
    def _lay_out(self) -> List[dict]:
        """One dict per layer: its kind, variable scope, sizes and the (H, W, C) of maps and mask before and after."""
        h, w, c = self.image_height, self.image_width, self.pixel_dim
        mh, mw = h, w
        plan = []
        for i, spec in enumerate(self.convolutions):
            kind = spec[0]
            layer = {"kind": kind, "index": i, "in": (h, w, c), "mask_in": (mh, mw)}
            if kind == "C":
                if not matches(spec, ConvSpec):                                              # :215-222
                    raise ValueError((
                        "Specification of a convolutional layer (number {} in config) "
                        'needs to have 5 members: "C", kernel size, stride, '
                        "padding, output channels, was {}").format(i, spec))
                k, stride, pad, out_channels = spec[1:]
                _check_padding(pad, i)                                                       # :225-228
                layer.update(scope="convolutions/layer_{}_convolution".format(i), k=k, stride=stride, pad=pad)
                oh, ow = ops.conv2d_out_hw(h, w, k, pad)                                     # the stride is not passed on
                mh, mw = ops.window2d_out_hw(mh, mw, (k, k), (stride, stride), pad)          # ... but pools the mask
                h, w, c = oh, ow, out_channels
            elif kind in ["M", "A"]:
                if not matches(spec, MaxPoolSpec):                                           # :294-300
                    raise ValueError((
                        "Specification of a max-pooling layer (number {} in config) "
                        'needs to have 3 members: "M", pool size, stride, padding, '
                        "was {}").format(i, spec))
                _, size, stride, pad = spec
                _check_padding(pad, i)                                                       # :312-315
                layer.update(size=size, stride=stride)                                       # the padding is not passed on
                h, w = ops.window2d_out_hw(h, w, (size, size), (stride, stride), "valid")
                mh, mw = ops.window2d_out_hw(mh, mw, (size, size), (stride, stride), "valid")
            elif kind == "R":
                if not self.batch_normalize:                                                 # :138-141
                    raise ValueError(
                        "Using ResNet blocks requires batch normalization "
                        "to be turned on.")
                if not matches(spec, ResNetSpec):                                            # :251-257
                    raise ValueError((
                        "Specification of a residual block (number {} in config) "
                        'needs to have 3 members: "R", kernel size, channels; '
                        "was {}").format(i, spec))
                k, out_channels = spec[1:]
                layer.update(scope="convolutions/layer_{}_resnet_block".format(i), k=k, project=out_channels != c)
                c = out_channels
            else:                                                                            # :149-151
                raise ValueError(
                    "Unknown type of convoutional layer #{}: '{}'".format(
                        i + 1, kind))
            if min(h, w, mh, mw) < 1:
                raise ValueError("CNNEncoder '{}': layer {} ({}) leaves no map: {} x {} after it, mask {} x {}"
                                 .format(self.name, i, spec, h, w, mh, mw))
            if (h, w) != (mh, mw):
                raise ValueError("CNNEncoder '{}': after layer {} ({}) the states are {} x {} and the mask is {} x {}"
                                 .format(self.name, i, spec, h, w, mh, mw))
            layer.update(out=(h, w, c), mask_out=(mh, mw))
            plan.append(layer)
        if not plan:
            raise ValueError("CNNEncoder '{}': no layers".format(self.name))
        return plan

    @property
    def input_types(self) -> Dict[str, type]:
        return {self.data_id: np.float32}

    @property
    def input_shapes(self) -> Dict[str, List]:
        return {self.data_id: [None, self.image_height, self.image_width, self.pixel_dim]}

    @property
    def spatial_shape(self) -> Tuple[int, int, int]:
        """(H', W', C') of the last map."""
        return self._plan[-1]["out"]

    @property
    def dimension(self) -> int:
        return self.spatial_shape[2]

    @property
    def output_size(self) -> int:
        return self.fully_connected[-1] if self.fully_connected else self.spatial_shape[2]

    def graph_safe_training(self, train_mode: bool) -> bool:
        """The forward pass of a training step writes the moving statistics: a replay would be correct, but the step
        is not worth a graph (a dozen launches), and the images are staged from the host on every step anyway.
        Under data parallelism it MUST stay False: every batch-norm layer then exchanges its statistics (forward) and its
        two channel sums (backward) with the other ranks (image_ops.batch_norm2d), the backward pass waits on the host
        for the global row count, and neither a collective nor a host wait may land inside a captured step graph."""
        return False

    # -- variables ---------------------------------------------------------------------------------------------
    def _declare_conv(self, store, scope: str, k: int, cin: int, cout: int) -> None:
        # tf.layers.conv2d: glorot uniform with the fans of a [k, k, in, out] filter, zero bias
        self.declare(store, scope + "/conv2d/kernel", (k, k, cin, cout), conv_filter_initializer())
        self.declare(store, scope + "/conv2d/bias", (cout,), zeros_initializer())

    def _declare_bn(self, store, scope: str, c: int) -> None:
        if not self.batch_normalize:
            return
        pre = scope + "/batch_normalization/"
        self.declare(store, pre + "gamma", (c,), ones_initializer())
        self.declare(store, pre + "beta", (c,), zeros_initializer())
        self.declare(store, pre + "moving_mean", (c,), zeros_initializer(), trainable=False)
        self.declare(store, pre + "moving_variance", (c,), ones_initializer(), trainable=False)

    def declare_variables(self, store) -> None:
        for layer in self._plan:
            cin, cout = layer["in"][2], layer["out"][2]
            if layer["kind"] == "C":
                self._declare_conv(store, layer["scope"], layer["k"], cin, cout)
                self._declare_bn(store, layer["scope"], cout)
            elif layer["kind"] == "R":
                scope = layer["scope"]
                if layer["project"]:
                    self._declare_conv(store, scope + "/project_input", 1, cin, cout)
                    self._declare_bn(store, scope + "/project_input", cout)
                self._declare_bn(store, scope + "/conv_a", cin)
                self._declare_conv(store, scope + "/conv_a", layer["k"], cin, cout)
                self._declare_bn(store, scope + "/conv_b", cout)
                self._declare_conv(store, scope + "/conv_b", layer["k"], cout, cout)
        if self.fully_connected is not None:
            h, w, c = self.spatial_shape
            mlp.declare_multilayer_projection(self, store, MLP_SCOPE, h * w * c, self.fully_connected)

    # -- inputs -------------------------------------------------------------------------------------------------
    def feed_dict(self, dataset, train: bool = False) -> FeedDict:
        fd = ModelPart.feed_dict(self, dataset, train)
        # if it is from the pickled file, it is a list, not a numpy tensor (:202-205)
        images = np.array(list(dataset.get_series(self.data_id)))
        fd[self.image_input] = (images / 255.0).astype(np.float32)
        return fd

    @tensor
    def image_input_tensor(self, ctx) -> torch.Tensor:
        """The fed images in a persistent device buffer."""
        images = ctx.fed(self.image_input)
        want = (self.image_height, self.image_width, self.pixel_dim)
        if tuple(images.shape[1:]) != want:
            raise ValueError("CNNEncoder '{}': fed images of shape {}, expected {}"
                             .format(self.name, tuple(images.shape[1:]), want))
        return ctx.session.staged((id(self), "images"), ctx.session.to_device(images, torch.float32, "image_input"))

    @tensor
    def image_mask(self, ctx) -> torch.Tensor:
        """sign(sum over the channels) of the fed images, [B, H, W, 1] (:103), derived on the host."""
        images = ctx.fed(self.image_input)
        return ctx.session.staged((id(self), "image_mask"), ctx.session.to_device(
            images, torch.float32, "image_mask",
            lambda im: np.sign(np.asarray(im, np.float32).sum(axis=3, keepdims=True, dtype=np.float32))))

    def stage_inputs(self, ctx) -> None:
        self.image_input_tensor(ctx)
        self.image_mask(ctx)

    # -- forward ------------------------------------------------------------------------------------------------
    def _conv(self, tape, x, scope: str, shape, pad: str):
        return I.conv2d(tape, x, tape.param(self, scope + "/conv2d/kernel"), tape.param(self, scope + "/conv2d/bias"),
                        shape, pad)

    def _bn(self, ctx, tape, x, scope: str, train: bool, relu: bool, stats: dict):
        """batch_norm_callback (:105-109) and the ReLU after it; without batch normalisation the ReLU alone."""
        if not self.batch_normalize:
            return F.relu(tape, x) if relu else x
        pre = scope + "/batch_normalization/"
        out, (mean, var) = I.batch_norm2d(
            tape, x, tape.param(self, pre + "gamma"), tape.param(self, pre + "beta"), self.var(ctx, pre + "moving_mean"),
            self.var(ctx, pre + "moving_variance"), train, relu,
            update_moving=train and bool(ctx.memo.get("want_backward", False)))
        stats[pre + "batch_mean"], stats[pre + "batch_variance"] = mean, var
        return out

    def _pool_mask(self, ctx, mask, index: int, window, stride, pad: str) -> torch.Tensor:
        bsz, mh, mw, _ = mask.shape
        oh, ow = ops.window2d_out_hw(mh, mw, window, stride, pad)
        out = ctx.buffer((id(self), "mask", index, bsz), (bsz, oh, ow, 1))
        return I.window2d_mask(mask, out, window, stride, pad)

    @tensor
    def _activations(self, ctx):
        train = bool(ctx.fed(self.train_mode))
        images = self.image_input_tensor(ctx)
        mask = self.image_mask(ctx)
        bsz = images.shape[0]
        tape = F.Tape(ctx, (id(self), "cnn"), recording=ctx.wants_backward(train))
        shape = (bsz, self.image_height, self.image_width)
        x = tape.leaf(images.view(bsz * shape[1] * shape[2], self.pixel_dim))
        layers, stats = [], {}
        for layer in self._plan:
            i, kind = layer["index"], layer["kind"]
            if kind == "C":
                k, stride, pad = layer["k"], layer["stride"], layer["pad"]
                x, shape = self._conv(tape, x, layer["scope"], shape, pad)
                x = self._bn(ctx, tape, x, layer["scope"], train, True, stats)
                mask = self._pool_mask(ctx, mask, i, (k, k), (stride, stride), pad)
            elif kind in ("M", "A"):
                win, stride = (layer["size"],) * 2, (layer["stride"],) * 2
                x, shape = I.window2d(tape, "max" if kind == "M" else "avg", x, shape, win, stride, "valid")
                mask = self._pool_mask(ctx, mask, i, win, stride, "valid")
            else:
                scope = layer["scope"]
                before = x
                if layer["project"]:                                                         # :264-268
                    before, _ = self._conv(tape, x, scope + "/project_input", shape, "same")
                    before = self._bn(ctx, tape, before, scope + "/project_input", train, False, stats)
                after = self._bn(ctx, tape, x, scope + "/conv_a", train, True, stats)        # :270-275
                after, _ = self._conv(tape, after, scope + "/conv_a", shape, "same")
                after = self._bn(ctx, tape, after, scope + "/conv_b", train, True, stats)    # :277-282
                after, _ = self._conv(tape, after, scope + "/conv_b", shape, "same")
                x = F.add(tape, after, before)                                               # :284
            layers.append((x, mask, shape))
        h, w, c = self.spatial_shape
        assert shape == (bsz, h, w) and tuple(mask.shape) == (bsz, h, w, 1), (shape, tuple(mask.shape))
        if self.fully_connected is None:
            out, _ = I.window2d(tape, "avg", x, shape, (h, w), (1, 1), "valid")              # tf.reduce_mean(., [1, 2])
        else:
            flat = tape.view(x, lambda t: t.view(bsz, h * w * c))
            out = mlp.multilayer_projection(tape, ctx, self, MLP_SCOPE, flat, self.fully_connected, "relu",
                                            self.dropout_keep_prob, train)
        return {"tape": tape, "states": x, "mask": mask, "output": out, "layers": layers, "stats": stats,
                "shape": (bsz, h, w, c)}

    @tensor
    def image_processing_layers(self, ctx) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """[(map [B, H_i, W_i, C_i], mask [B, H_i, W_i, 1])] after every layer."""
        return [(var.data.view(shape + (var.shape[1],)), mask) for var, mask, shape in self._activations(ctx)["layers"]]

    @tensor
    def batch_statistics(self, ctx) -> Dict[str, torch.Tensor]:
        """``<scope>/batch_normalization/batch_{mean,variance}`` of a training-mode pass (the biased variance)."""
        return self._activations(ctx)["stats"]

    @tensor
    def spatial_states(self, ctx) -> torch.Tensor:
        act = self._activations(ctx)
        return act["states"].data.view(act["shape"])

    @tensor
    def spatial_mask(self, ctx) -> torch.Tensor:
        return self._activations(ctx)["mask"]

    @tensor
    def output(self, ctx) -> torch.Tensor:
        return self._activations(ctx)["output"].data

    def backward(self, ctx, d_states: Optional[torch.Tensor], d_final: Optional[torch.Tensor] = None) -> None:
        """dL/d(spatial_states) [B, H', W', C'] (any shape with those elements) and dL/d(output)."""
        act = self._activations(ctx)
        tape = act["tape"]
        if not tape.recording:
            raise RuntimeError("CNNEncoder.backward needs a run with train_mode=True")
        bsz, h, w, c = act["shape"]
        if d_states is not None:
            ops.ew("copy", d_states.reshape(bsz * h * w, c), None, tape.grad(act["states"]), accumulate=True)
        if d_final is not None:
            ops.ew("copy", d_final, None, tape.grad(act["output"]), accumulate=True)
        tape.backward()


class CNNTemporalView(ModelPart, TemporalStatefulWithOutput):
    """Slice the convolutional maps left to right."""
    has_time_loop = False

    def __init__(self,
                 name: str,
                 cnn: CNNEncoder) -> None:
        check_argument_types()
        ModelPart.__init__(self, name, save_checkpoint=None, load_checkpoint=None)
        self._cnn = cnn

    @property
    def dependencies(self) -> List[str]:
        return super().dependencies + ["_cnn"]

    @property
    def dimension(self) -> int:
        h, _, c = self._cnn.spatial_shape
        return h * c

    @property
    def output_size(self) -> int:
        return self._cnn.output_size

    def graph_safe_training(self, train_mode: bool) -> bool:
        return False

    @tensor
    def output(self, ctx) -> torch.Tensor:
        return self._cnn.output(ctx)

    @tensor
    def temporal_states(self, ctx) -> torch.Tensor:
        """tf.transpose(spatial_states, [0, 2, 1, 3]) reshaped to [B, W', H'*C'] (:340-344): one launch."""
        states = self._cnn.spatial_states(ctx)                              # [B, H', W', C']
        bsz, h, w, c = states.shape
        return ops.map_columns(states, ctx.buffer((id(self), "temporal_states", bsz), (bsz, w, h * c)))

    @tensor
    def temporal_mask(self, ctx) -> torch.Tensor:
        """(sum over H' of the mask) > 0 as floats (:348-350): for a 0/1 mask its maximum over H', the pooling kernel
        with a window of the whole height."""
        mask = self._cnn.spatial_mask(ctx)                                  # [B, H', W', 1]
        bsz, h, w, _ = mask.shape
        out = ctx.buffer((id(self), "temporal_mask", bsz), (bsz, 1, w, 1))
        I.window2d_mask(mask, out, (h, 1), (1, 1), "valid")
        return out.view(bsz, w)

    @tensor
    def lengths(self, ctx) -> torch.Tensor:
        """int32 [B]: the sum of ``temporal_mask``, what the reference's recurrent encoder takes as lengths."""
        mask = self.temporal_mask(ctx)
        return ops.ctc_mask_lengths(mask, ctx.buffer((id(self), "lengths", mask.shape[0]), (mask.shape[0],), torch.int32))

    def backward(self, ctx, d_states: Optional[torch.Tensor], d_final: Optional[torch.Tensor] = None) -> None:
        """dL/d(temporal_states) [B, W', H'*C'] back into the map's layout; both gradients go to the CNN through
        ``defer_backward``, so a CNN read by this view and by others replays its tape once."""
        d_map = None
        if d_states is not None:
            h, w, c = self._cnn.spatial_shape
            bsz = d_states.shape[0]
            d_map = ops.map_columns(d_states.reshape(bsz, w, h * c).contiguous(),
                                    ctx.buffer((id(self), "d_map", bsz), (bsz, h, w, c)), inverse=True)
        if d_map is not None or d_final is not None:
            ctx.defer_backward(self._cnn, d_map, d_final)
