"""Taped functions of the image stack (csrc/nm_image.hip) for ``autodiff.Tape``: tf.layers.conv2d, batch normalisation
(+ ReLU) and the pooling windows of neuralmonkey/encoders/cnn_encoder.py.

A map lives on the tape as the 2-D Var [B*H*W, C] of its NHWC rows (what every other taped function expects: ``relu``,
``add``, ``linear`` over the flattened map are plain row operations); the functions here take the map's (B, H, W)
alongside and return the output's.  Like the functions of ``autodiff`` each launches its forward kernel(s) now and, on a
recording tape, appends a closure that launches the gradient kernels; gradients accumulate through ``Tape.grad_slot``.
"""
from typing import Tuple

import torch

from . import ops
from .autodiff import Tape, Var

Shape3 = Tuple[int, int, int]


def _map(t: torch.Tensor, shape: Shape3) -> torch.Tensor:
    bsz, h, w = shape
    assert t.dim() == 2 and t.shape[0] == bsz * h * w and t.is_contiguous(), (tuple(t.shape), shape)
    return t.view(bsz, h, w, t.shape[1])


def conv2d(tape: Tape, x: Var, filt: Var, bias: Var, shape: Shape3, padding: str, algo: int = 0):
    """tf.layers.conv2d(x, Cout, k, padding=padding, activation=None) at stride 1 (cnn_encoder.py:231, :265, :273, :280)
    over x [B*H*W, Cin] with filt [k, k, Cin, Cout]: one launch (nm_conv2d_fwd).  -> (y [B*OH*OW, Cout], (B, OH, OW)).
    Backward: nm_conv2d_bwd -- the data gradient as the transposed convolution, the filter and bias gradients by
    fixed-order slabs."""
    bsz, h, w = shape
    k, cin, cout = int(filt.shape[0]), int(filt.shape[2]), int(filt.shape[3])
    oh, ow = ops.conv2d_out_hw(h, w, k, padding)
    if oh < 1 or ow < 1:
        raise ValueError("a {} x {} map is smaller than the {} x {} filter of a 'valid' convolution".format(h, w, k, k))
    out = tape.new((bsz * oh * ow, cout))
    out_shape = (bsz, oh, ow)
    x4 = _map(x.data, shape)
    ops.conv2d_fwd(x4, filt.data, bias.data, _map(out.data, out_shape), padding, algo=algo)

    def bwd():
        if out.grad is None:
            return
        gx, acc = tape.grad_slot(x) if x.needs_grad else (None, False)
        want_params = filt.needs_grad or bias.needs_grad
        ws = tape.buf((max(1, ops.conv2d_workspace_floats(bsz, h, w, cin, k, cout, padding)),)) if want_params else None
        ops.conv2d_bwd(x4, filt.data, _map(out.grad, out_shape), padding, dx=None if gx is None else _map(gx, shape),
                       accumulate_dx=acc, dfilt=tape.grad(filt) if filt.needs_grad else None,
                       dbias=tape.grad(bias) if bias.needs_grad else None, accumulate_params=True, workspace=ws,
                       algo=algo)
    tape.record(bwd)
    return out, out_shape


def batch_norm2d(tape: Tape, x: Var, gamma: Var, beta: Var, moving_mean: torch.Tensor, moving_var: torch.Tensor,
                 training: bool, relu: bool, update_moving: bool = False):
    """tf.layers.batch_normalization(x, training=training) with TensorFlow's defaults over the rows of x [B*H*W, C]
    (cnn_encoder.py:107), and the ReLU that follows it everywhere but in ``project_input`` (nm_bn2d_fwd).  Training:
    the batch's mean and biased variance, kept for the backward pass; ``update_moving``: the moving statistics take
    their step (what the trainers' UPDATE_OPS fetch does, generic_trainer.py:250).  Inference: the moving statistics.
    -> (y, (batch mean, batch variance) -- None, None in inference).  Backward (training mode only): nm_bn2d_bwd.

    Training under data parallelism (a ``distributed.DataParallel`` of several ranks, or a forced one, is current): the
    statistics are those of ALL ranks' rows -- ``_batch_norm2d_over_ranks``.  Inference never exchanges anything."""
    from . import distributed
    dp = distributed.current()
    if training and dp is not None and (dp.world_size > 1 or dp.forced):
        return _batch_norm2d_over_ranks(tape, dp, x, gamma, beta, moving_mean, moving_var, relu, update_moving)
    c = x.shape[1]
    out = tape.new(tuple(x.shape))
    mean = tape.buf((c,)) if training else None
    var = tape.buf((c,)) if training else None
    ops.bn2d_fwd(x.data, gamma.data, beta.data, out.data, training, relu,
                 moving_mean=moving_mean if (update_moving or not training) else None,
                 moving_var=moving_var if (update_moving or not training) else None, batch_mean=mean, batch_var=var)

    def bwd():
        if out.grad is None:
            return
        if not training:
            raise NotImplementedError("batch_norm2d: the backward pass exists in training mode only")
        gx, acc = tape.grad_slot(x) if x.needs_grad else (None, False)
        ops.bn2d_bwd(x.data, out.data if relu else None, out.grad, gamma.data, mean, var, relu, tape.buf((2 * c,)),
                     dx=gx, accumulate_dx=acc, dgamma=tape.grad(gamma) if gamma.needs_grad else None,
                     dbeta=tape.grad(beta) if beta.needs_grad else None, accumulate_params=True)
    tape.record(bwd)
    return out, (mean, var)


def _batch_norm2d_over_ranks(tape: Tape, dp, x: Var, gamma: Var, beta: Var, moving_mean: torch.Tensor,
                             moving_var: torch.Tensor, relu: bool, update_moving: bool):
    """Training-mode ``batch_norm2d`` whose batch is dealt over the ranks of ``dp`` (include/nmhip_bnsync.h); the ranks'
    row counts may differ.  Forward: nm_bn2d_part_stats -> the parts of all ranks gathered -> nm_bn2d_merge (every rank
    merges the same parts in rank order: identical batch and moving statistics everywhere) -> nm_bn2d_fwd in inference
    mode on the merged statistics.  Backward: nm_bn2d_bwd_sums (dgamma / dbeta take the rank's OWN sums: the gradient
    exchange adds the ranks' up) -> the [2C] sums added over the ranks -> nm_bn2d_bwd_dx with the global row count.
    Two exchanges per layer and step, issued where the tape stands: every rank runs the same tape in the same order."""
    c = x.shape[1]
    out = tape.new(tuple(x.shape))
    mean, var = tape.buf((c,)), tape.buf((c,))
    part = tape.buf((ops.bn2d_part_doubles(c),), torch.float64)
    total = tape.buf((1,), torch.float64)
    ops.bn2d_part_stats(x.data, part)
    ops.bn2d_merge(dp.gather_parts(part), mean, var, total, moving_mean=moving_mean if update_moving else None,
                   moving_var=moving_var if update_moving else None)
    ops.bn2d_fwd(x.data, gamma.data, beta.data, out.data, False, relu, moving_mean=mean, moving_var=var)
    rows = dp.read_later(total) if tape.recording else None      # (the backward pass needs the count on the host)

    def bwd():
        if out.grad is None:
            return
        sums = tape.buf((2 * c,))
        ops.bn2d_bwd_sums(x.data, out.data if relu else None, out.grad, mean, var, relu, sums,
                          dgamma=tape.grad(gamma) if gamma.needs_grad else None,
                          dbeta=tape.grad(beta) if beta.needs_grad else None, accumulate_params=True)
        if not x.needs_grad:
            return
        dp.sum_small(sums)
        gx, acc = tape.grad_slot(x)
        ops.bn2d_bwd_dx(x.data, out.data if relu else None, out.grad, gamma.data, mean, var, relu, sums, int(rows()), gx,
                        accumulate_dx=acc)
    tape.record(bwd)
    return out, (mean, var)


def window2d(tape: Tape, mode: str, x: Var, shape: Shape3, window: Tuple[int, int], stride: Tuple[int, int],
             padding: str = "valid"):
    """tf.layers.max_pooling2d / average_pooling2d (cnn_encoder.py:318) over x [B*H*W, C] (nm_window2d_fwd); with the
    window (H, W) and "avg" it is tf.reduce_mean(x, [1, 2]) (:187).  -> (y [B*OH*OW, C], (B, OH, OW)).  Backward:
    nm_window2d_bwd -- the maximum's gradient goes to the first maximum of a window."""
    bsz, h, w = shape
    c = x.shape[1]
    oh, ow = ops.window2d_out_hw(h, w, window, stride, padding)
    if oh < 1 or ow < 1:
        raise ValueError("a {} x {} map is smaller than the {} x {} window of a 'valid' pooling".format(h, w, *window))
    out_shape = (bsz, oh, ow)
    out = tape.new((bsz * oh * ow, c))
    argmax = tape.buf((bsz * oh * ow, c), torch.int32) if (mode == "max" and tape.recording) else None
    ops.window2d_fwd(mode, _map(x.data, shape), _map(out.data, out_shape), window, stride, padding, argmax=argmax)

    def bwd():
        if out.grad is None or not x.needs_grad:
            return
        gx, acc = tape.grad_slot(x)
        ops.window2d_bwd(mode, _map(out.grad, out_shape), _map(gx, shape), window, stride, padding, argmax=argmax,
                         accumulate=acc)
    tape.record(bwd)
    return out, out_shape


def window2d_mask(mask: torch.Tensor, out: torch.Tensor, window: Tuple[int, int], stride: Tuple[int, int],
                  padding: str) -> torch.Tensor:
    """tf.layers.max_pooling2d of the [B, H, W, 1] mask (cnn_encoder.py:238, :319): the same kernel with C = 1 and no
    gradient."""
    return ops.window2d_fwd("max", mask, out, window, stride, padding)
